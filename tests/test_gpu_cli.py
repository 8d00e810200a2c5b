"""End-to-end CLI surface on the GPU: config.ini read from the CWD, dataset directory as argv[1], the reference's
progress lines, a checkpoint per global epoch and `to_restore` (Codes/train.py:359-381, :45-48, :354)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIG = """[Long-Tail-GAN]
h0_size = 100
h1_size = 150
h2_size = 250
h3_size = 300
NUM_EPOCH = {num_epoch}
BATCH_SIZE = 100
DISPLAY_ITER = 50
LEARNING_RATE = 0.0001
to_restore = {to_restore}
model_name = LT_GAN
GANLAMBDA = 1.0
"""


def test_train_cli_two_epochs_and_resume(tmp_path):
    from ltgan.dataset import materialize_askubuntu
    ds = str(tmp_path / "Askubuntu_Sample")
    materialize_askubuntu(os.path.join(ROOT, "tests", "golden", "askubuntu_raw.npz"), ds)
    cwd = str(tmp_path / "run")
    os.makedirs(cwd)
    script = os.path.join(ROOT, "long-tail-gan_amd", "train.py")
    # NUM_EPOCH = 2 global epochs... NUM_SUB_EPOCHS = int(2/8) = 0 would skip the D/G phases, so use 8 -> 1 sub-epoch
    # and stop after two global epochs through the environment knob of the test harness
    open(os.path.join(cwd, "config.ini"), "w").write(CONFIG.format(num_epoch=8, to_restore=0))
    env = dict(os.environ, LTGAN_MAX_EPOCHS="2")
    out = subprocess.run([sys.executable, script, ds], cwd=cwd, capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    txt = out.stdout
    assert "Number of Users:  10001" in txt and "Batches Per Epoch:  101" in txt
    assert "global-epoch: 0 Data Creation Finished user_err_cnt: 468" in txt          # Q8: 10001 - 9533 invalid users
    assert "global-epoch:0, discr-epoch:0, d_loss:" in txt and "global-epoch:1, generator-epoch:0, g_loss:" in txt
    ndcg = [float(l.split("NDCG:")[1].split()[0]) for l in txt.splitlines() if "Vad: NDCG:" in l]
    assert len(ndcg) == 2 and 0.15 < ndcg[0] < 0.5 and ndcg[1] > ndcg[0] - 0.01      # learning, same ballpark as the oracle run
    ck = os.path.join(cwd, "chkpt", "Askubuntu_Sample_LT_GAN_1.0")
    assert sorted(os.listdir(ck)) == ["model_0.pt", "model_1.pt"]
    # resume: to_restore = 1 continues at global epoch 2
    open(os.path.join(cwd, "config.ini"), "w").write(CONFIG.format(num_epoch=8, to_restore=1))
    env = dict(os.environ, LTGAN_MAX_EPOCHS="1")
    out = subprocess.run([sys.executable, script, ds], cwd=cwd, capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "Restored" in out.stdout and "global-epoch: 2 Data Creation Finished" in out.stdout
    assert "model_2.pt" in os.listdir(ck)
    # test.py: restore -> chunked scoring -> "NDCG@100<TAB>R@20<TAB>R@50" (Codes/test.py:134-173)
    tscript = os.path.join(ROOT, "long-tail-gan_amd", "test.py")
    out = subprocess.run([sys.executable, tscript, ds, os.path.join(ck, "model_2.pt")], cwd=cwd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "Model Loaded" in out.stdout
    vals = [float(x) for x in out.stdout.strip().splitlines()[-1].split("\t")]
    assert len(vals) == 3 and 0.15 < vals[0] < 0.5 and 0.0 < vals[1] <= vals[2] <= 1.0
    # the same under torchrun (2 ranks, item-sharded): same numbers up to all-reduce order
    env2 = dict(os.environ, LTGAN_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29633", tscript, ds, os.path.join(ck, "model_2.pt")]
    out2 = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, env=env2, timeout=1200)
    assert out2.returncode == 0, out2.stdout[-2000:] + out2.stderr[-4000:]
    vals2 = [float(x) for x in [l for l in out2.stdout.strip().splitlines() if l.count("\t") == 2][-1].split("\t")]
    assert max(abs(a - b) for a, b in zip(vals, vals2)) < 3e-3


def test_train_cli_needs_config_in_cwd(tmp_path):
    script = os.path.join(ROOT, "long-tail-gan_amd", "train.py")
    out = subprocess.run([sys.executable, script, "/nonexistent"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "config.ini" in out.stderr


def test_train_cli_under_torchrun_item_sharded(tmp_path):
    """Two ranks (gloo, both on the one GPU of the test box) run the same CLI: rank 0 prints the reference's lines,
    the checkpoint holds FULL tensors, and a single-process run resumes from it (world-size independent format)."""
    import torch
    from ltgan.dataset import materialize_askubuntu
    ds = str(tmp_path / "Askubuntu_Sample")
    materialize_askubuntu(os.path.join(ROOT, "tests", "golden", "askubuntu_raw.npz"), ds)
    cwd = str(tmp_path / "run")
    os.makedirs(cwd)
    script = os.path.join(ROOT, "long-tail-gan_amd", "train.py")
    open(os.path.join(cwd, "config.ini"), "w").write(CONFIG.format(num_epoch=8, to_restore=0))
    env = dict(os.environ, LTGAN_MAX_EPOCHS="1", LTGAN_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29631", script, ds]
    out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, env=env, timeout=1200)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    txt = out.stdout
    assert txt.count("global-epoch: 0 Data Creation Finished user_err_cnt: 468") == 1           # rank 0 only
    ndcg = [float(l.split("NDCG:")[1].split()[0]) for l in txt.splitlines() if "Vad: NDCG:" in l]
    assert len(ndcg) == 1 and 0.15 < ndcg[0] < 0.5
    ck = os.path.join(cwd, "chkpt", "Askubuntu_Sample_LT_GAN_1.0", "model_0.pt")
    st = torch.load(ck, map_location="cpu", weights_only=True)      # tensors and plain numbers only: no pickled objects in a model file
    assert not [f for f in os.listdir(os.path.dirname(ck)) if ".tmp" in f]          # written to a temporary, renamed into place
    for k in ("weight_q_0to1", "weight_q_0to1/Adam_1"):
        assert tuple(st[k].shape) == (1000, 600), k
    for k in ("weight_p_1to2", "weight_p_1to2/Adam"):                               # TF shape of the reference variable: [600, n_items]
        assert tuple(st[k].shape) == (600, 1000), k
    assert st["format"] == 3 and st["shuffle_rng_state"][0] == "MT19937" and tuple(st["shuffle_rng_state"][1].shape) == (624,)
    assert tuple(st["bias_p_2"].shape) == (1000,) and float(st["weight_p_1to2/Adam_1"].abs().sum()) > 0
    open(os.path.join(cwd, "config.ini"), "w").write(CONFIG.format(num_epoch=8, to_restore=1))
    env = dict(os.environ, LTGAN_MAX_EPOCHS="1")
    out = subprocess.run([sys.executable, script, ds], cwd=cwd, capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "Restored" in out.stdout and "global-epoch: 1 Data Creation Finished" in out.stdout


def test_bench_dump_outputs_of_the_timed_step(tmp_path):
    """--dump-outputs DIR: after the timed steps bench.py writes the last step's losses, fake pairs and model tensors as float32 .npy files
    (under 64 MB), and --steps sets the number of timed steps that ms_per_step divides."""
    import json
    import numpy as np
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--sub-epochs", "2", "--no-probe",
                          "--no-cpu-baseline", "--no-other-workloads", "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 - d["config"]["users"]) < 1e-6 * d["config"]["users"]
    files = {p.name: np.load(p) for p in (tmp_path / "dump").iterdir()}
    assert {"d_losses.npy", "g_losses.npy", "fake_cnt.npy", "fake_gen.npy", "gen_W_q0.npy", "disc_0.npy"} <= set(files)
    assert all(x.dtype == np.float32 for x in files.values()) and sum(x.nbytes for x in files.values()) <= 64 << 20
    assert files["d_losses.npy"].shape == (2, 8) and np.all(np.isfinite(files["d_losses.npy"][:, 0])) and np.all(np.isfinite(files["g_losses.npy"][:, :3]))
    assert files["fake_cnt.npy"].shape == (d["config"]["batches"],) and files["fake_cnt.npy"].sum() > 0
    assert files["gen_W_q0.npy"].shape[1] == 600 and np.all(np.isfinite(files["gen_W_q0.npy"]))


def test_bench_plain_run_measures_the_headline_alone():
    """Without --full bench.py runs nothing of its own beside the timed steps: the line carries the headline keys and the roofline of the
    kernels probed inside the run, and none of the CPU baseline, the other workloads, the per-rank proxy or the copy ceiling."""
    import json
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--sub-epochs", "2"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config", "roofline"):
        assert k in d, k
    assert d["unit"] == "users/s" and d["higher_is_better"] is True and d["dtype"] == "bf16" and d["config"]["workload"] == "askubuntu"
    assert abs(d["ms_per_step"] * 1e-3 * d["value"] - d["config"]["users"]) < 1e-3 * d["config"]["users"]
    for k in ("cpu_baseline", "other_workloads", "projected_strong_scaling_8gpu_upper_bound", "c4_same_workload"):
        assert k not in d, k
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and "copy_ceiling_this_box" not in r and r["frac_of_copy_ceiling"] is None


def test_bench_contract_one_json_line():
    """bench.py --full prints ONE JSON line (the last line of stdout) carrying the driver's keys plus roofline and cpu_baseline."""
    import json
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--sub-epochs", "2",
                          "--cpu-seconds", "3", "--full"], capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    line = out.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["warmup"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["unit"] == "users/s" and d["value"] > 1000 and d["config"]["workload"] == "askubuntu" and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] is None or r["traffic"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "users/s" and "sample" in c
    assert abs(d["ms_per_step"] * 1e-3 * d["value"] - d["config"]["users"]) < 1e-3 * d["config"]["users"]
    assert 0 < r["step_frac"] < 1 and r["step_algorithmic_bytes"] > 0
    ow = d["other_workloads"]
    assert ow["c3"]["items"] == 20000 and ow["c4"]["items"] == 200000 and ow["c3"]["value"] > 0 and ow["c4"]["value"] > 0
    assert ow["c4"]["dominant_kernel"]["bound"] == "hbm" and 0 < ow["c4"]["dominant_kernel"]["frac"] < 1
    # round 6: the arithmetic of the discriminator's products is named; `frac` follows from the tracked rocprofv3 summary when there is one
    # (both durations in the line); the dominant kernel BY TOTAL TIME of that summary with its own fraction; the per-rank proxy of an 8-GPU
    # run on RCCL at world size 1 and the scaling bound it gives
    assert d["config"]["d_arith"] in ("fp32", "bf16x6", "bf16x4")
    assert r["avg_us_event_bracket"] > 0 and "avg_us_rocprof" in r and "frac_source" in r
    if r["avg_us_rocprof"]:
        assert abs(r["frac"] - (r["algorithmic_bytes"] if r["bound"] == "hbm" else r["algorithmic_flops"]) / (r["avg_us_rocprof"] * 1e-6) /
                   (r["peak"] * (1e9 if r["bound"] == "hbm" else 1e12))) < 1e-6
        dom = r["dominant_by_total_time"]
        assert dom["kernel"] not in ("k_gate_wait", "k_gate_set") and 0 < dom["share_of_kernel_time"] < 1 and 0 < dom["frac"] < 1
    rp = ow["rank_proxy"]
    assert "error" not in rp, rp
    assert rp["items"] == 25024 and rp["one_call"] and rp["transport"] == "rccl-direct" and rp["rccl_ranks"] == 1
    assert rp["g_step_us"] > 0 and rp["d_step_us"] > 0 and set(rp["exchanges_us"]) == {"exch_h1", "exch_rowpart", "exch_dh2"}
    assert 0 < rp["step_frac_of_copy_ceiling"] < 1.2
    want = (ow["c4"]["g_step_us"] + ow["c4"]["d_step_us"]) / (rp["g_step_us"] + rp["d_step_us"])
    assert abs(d["projected_strong_scaling_8gpu_upper_bound"] - want) < 1e-9 and 1 < want < 8


def test_bench_two_ranks_item_sharded():
    """`python bench.py --gpus 2 --full` with no launcher around it: the parent starts two fresh rank processes itself (before it
    touches the GPU), the ranks run the N > 1 branch (rank-0 reference run, item-sharded loop, max over ranks) and the
    parent relays rank 0's ONE JSON line.  The test box has one GPU, so the parent picks gloo and the ranks share it."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LTGAN_DIST_BACKEND")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--users", "400", "--sub-epochs", "2", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1 and out.stdout.strip().splitlines()[-1] == lines[0], lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["workload"] == "c4" and d["config"]["items"] == 100032
    assert d["config"]["backend"].startswith("gloo") or d["config"]["backend"].startswith("nccl")
    assert d["value"] > 0 and d["n1_same_workload"]["value"] > 0 and d["strong_scaling_vs_1gpu"] > 0
    assert d["roofline"]["kernel"] == "dec1_bwd_adam" and d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["step_frac"] < 1


def test_bench_item_sharded_code_path_on_rccl_at_world_size_one():
    """The item-sharded trainer on the RCCL backend (what an 8-GPU job runs; a one-GPU box can only host world size 1): the three
    exchanges of a G step, the side streams (fake tower, decoder weight update), the spans of phase C and the lazy Adam clock on a
    25 024-item slab -- the slab one rank of an 8-GPU run of the 200 000-item configuration owns."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LTGAN_DIST_BACKEND")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "custom:25024", "--users", "400", "--steps", "1", "--warmup", "1", "--sub-epochs", "2",
           "--parallelism", "item-shard", "--no-cpu-baseline", "--no-other-workloads"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    d = json.loads([l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 1 and d["config"]["backend"].startswith("nccl") and d["config"]["parallelism"].startswith("item-shard x1")
    assert d["value"] > 0 and d["roofline"]["kernel"] == "dec1_bwd_adam"
