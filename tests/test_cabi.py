"""CPU-side checks of the drop-in boundary: the C-ABI library builds/loads and exports every symbol
include/ltg.h declares (no compute without a GPU), struct layouts match, argument validation
returns error codes instead of crashing, and the product path refuses to run without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "ltg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ltg_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_are_exported_and_bound():
    from ltgan import _cabi as cabi
    names = _declared()
    assert names == sorted(cabi.SYMBOLS), (names, sorted(cabi.SYMBOLS))
    lib = cabi.load()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.ltg_abi_version() == cabi.LTG_ABI_VERSION == 14


def test_struct_layouts_match_header():
    from ltgan import _cabi as cabi
    assert C.sizeof(cabi.ltg_config) == 80 and cabi.ltg_config.seed.offset == 72
    assert C.sizeof(cabi.ltg_gen_state) == 28 * 8 and cabi.ltg_gen_state.q0_ord.offset == 27 * 8 and C.sizeof(cabi.ltg_disc_state) == 30 * 8 and cabi.ltg_disc_state.emb_fp8.offset == 25 * 8 and cabi.ltg_disc_state.w3_fp8.offset == 29 * 8
    assert C.sizeof(cabi.ltg_batch) == 8 + 9 * 8 and cabi.ltg_batch.uitem.offset == 8 + 8 * 8 and C.sizeof(cabi.ltg_gen_acts) == 8 * 8
    assert C.sizeof(cabi.ltg_fwd_opts) == 8 + 8 + 3 * 8 + 8 and cabi.ltg_fwd_opts.rows_per_step.offset == 40
    assert C.sizeof(cabi.ltg_pairs) == 8 + 3 * 8
    assert C.sizeof(cabi.ltg_d_opts) == 8 + 8 + 7 * 8 + 8 + 8 + 8 and cabi.ltg_d_opts.sync.offset == 80
    assert C.sizeof(cabi.ltg_g_opts) == C.sizeof(cabi.ltg_fwd_opts) + 16 + 8 + 8 * 8 + 24 and cabi.ltg_g_opts.dec1_done.offset == C.sizeof(cabi.ltg_g_opts) - 24
    assert C.sizeof(cabi.ltg_sample_inputs) == 8 + 7 * 8 + 8 + 3 * 8 + 8
    assert C.sizeof(cabi.ltg_probe) == 8 + 16
    assert C.sizeof(cabi.ltg_comm) == 8 + 8 + 2 * 8 and cabi.ltg_comm.all_reduce.offset == 16
    assert C.sizeof(cabi.ltg_pipe) == 7 * 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 and cabi.ltg_pipe.shadow_out.offset == 104 and cabi.ltg_pipe.q0_mark.offset == 80 and cabi.ltg_pipe.next_nu.offset == 96 and cabi.ltg_pipe.caught_up.offset == 100 and cabi.ltg_pipe.tail_stream.offset == 72 and cabi.ltg_pipe.h1pre.offset == 32 and cabi.ltg_pipe.flags.offset == 56 and cabi.ltg_pipe.seq.offset == 60 and cabi.ltg_pipe.sync.offset == 64


def test_struct_layouts_match_the_header_as_gcc_lays_it_out(tmp_path):
    """The numbers above are the binding's; this compiles include/ltg.h with gcc and compares size and EVERY field offset of every struct
    the binding mirrors (a C host that includes the header and the ctypes binding must agree on the bytes)."""
    import ctypes as C
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from ltgan import _cabi as cabi
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    names = ["ltg_config", "ltg_gen_state", "ltg_disc_state", "ltg_batch", "ltg_gen_acts", "ltg_probe", "ltg_fwd_opts", "ltg_pairs", "ltg_d_opts",
             "ltg_g_opts", "ltg_sample_inputs", "ltg_comm", "ltg_pipe", "ltg_oneshot", "ltg_g_route_info", "ltg_d_route_info", "ltg_pipe_plan_info"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "ltg.h"', "int main(void) {"]
    for n in names:
        st = getattr(cabi, n)
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (n, n))
        for f in st._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (n, f[0], n, f[0]))
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for ln in out:
        if not ln.strip():
            continue
        n, f, v = ln.split()
        st = getattr(cabi, n)
        if f == "size":
            assert C.sizeof(st) == int(v), (n, C.sizeof(st), int(v))
        else:
            assert getattr(st, f).offset == int(v), (n, f, getattr(st, f).offset, int(v))
        seen += 1
    assert seen == sum(1 + len(getattr(cabi, n)._fields_) for n in names)


def test_argument_validation_returns_codes_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    good = cabi.ltg_config(1000, 600, 200, 1000, 100, 150, 250, 300, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
    assert lib.ltg_workspace_bytes(C.byref(good), 100, 2000) > 0
    bad = cabi.ltg_config(0, 600, 200, 1000, 100, 150, 250, 300, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
    assert lib.ltg_workspace_bytes(C.byref(bad), 100, 2000) == 0
    odd = cabi.ltg_config(1000, 602, 200, 1000, 100, 150, 250, 300, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)   # H % 4 != 0
    assert lib.ltg_workspace_bytes(C.byref(odd), 100, 2000) == 0
    # NULL structs -> LTG_EINVAL, before any HIP call
    assert lib.ltg_vae_forward(C.byref(good), None, None, None, None, None, None, 0, None) == -1
    assert lib.ltg_d_step(C.byref(good), None, None, None, None, None, None, 0, None) == -1
    assert lib.ltg_g_step(C.byref(good), None, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.ltg_d_grad(C.byref(good), None, None, None, 0, 0, None, None, None, 0, None) == -1
    assert lib.ltg_d_apply(C.byref(good), None, None, 1, None, None) == -1
    assert lib.ltg_d_grad_floats(C.byref(good)) == (161001 + 1 + 3) // 4 * 4 and lib.ltg_d_grad_floats(C.byref(bad)) == 0
    assert lib.ltg_sample_pairs(C.byref(good), None, None, None, None, None, None, None) == -1
    assert lib.ltg_rank_metrics(C.byref(good), None, None, None, 100, 20, 50, None, None) == -1
    assert lib.ltg_g_step_sharded(C.byref(good), None, None, None, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.ltg_g_step_sharded_ok(C.byref(good), None, 100) == 0 and lib.ltg_g_pipe_join(None, None) == -1
    assert lib.ltg_g_step_sharded_plan(C.byref(good), None, None, None) == 0
    assert lib.ltg_g_pipe_plan(C.byref(good), None, None, None, None) == 0
    assert lib.ltg_g_pipe_plan(C.byref(good), C.byref(cabi.ltg_gen_state()), C.byref(cabi.ltg_batch(n_rows=16)), C.byref(cabi.ltg_pipe()), None) == 0   # no *out
    assert lib.ltg_g_pipe_plan(C.byref(bad), C.byref(cabi.ltg_gen_state()), C.byref(cabi.ltg_batch(n_rows=16)), C.byref(cabi.ltg_pipe()), C.byref(cabi.ltg_pipe_plan_info())) == 0
    assert lib.ltg_g_route(C.byref(good), None, 100, None) == 0 and lib.ltg_g_route(C.byref(bad), C.byref(cabi.ltg_gen_state()), 100, C.byref(cabi.ltg_g_route_info())) == 0
    assert lib.ltg_d_route(C.byref(good), None, 100, 1, 0, None) == 0 and lib.ltg_d_route(C.byref(bad), C.byref(cabi.ltg_disc_state()), 100, 1, 0, C.byref(cabi.ltg_d_route_info())) == 0
    # ltg_config.d_arith (ABI v14): 0 / 1 / 2 + the measurement set in bits 4-7; anything else is rejected
    for code, ok in ((0, True), (1, True), (2, True), (1 | (0xE << 4), True), (3, False), (1 | (1 << 8), False), (-1, False)):
        c = cabi.ltg_config(1000, 600, 200, 1000, 100, 150, 250, 300, 0, 0, 0, 0, 1, code, 1e-4, 0.9, 0.999, 1e-8, 1)
        assert (lib.ltg_workspace_bytes(C.byref(c), 100, 2000) > 0) == ok, code
    # ltg_config.tuning: the selection bits 14, 17-22 and 26; a retired measurement bit (0-3, 9, 12, 24, 27) or one never assigned (7) is refused
    kept = [1 << b for b in (14, 17, 18, 19, 20, 21, 22, 26)] + [(1 << 18) | (1 << 20)]
    for bits, ok in [(0, True)] + [(b, True) for b in kept] + [(b, False) for b in (1, 9, 1 << 7, 1 << 9, 1 << 12, 1 << 24, 1 << 27, -1)]:
        c = cabi.ltg_config(1000, 600, 200, 1000, 100, 150, 250, 300, 0, bits, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
        assert (lib.ltg_workspace_bytes(C.byref(c), 100, 2000) > 0) == ok, bits
    # ltg_pipe.flags: the LTG_PIPE_* switches only (the plan of a call that would be refused is 0); host-side checks, no pointer is read
    sh = cabi.ltg_config(8192, 600, 200, 1000, 100, 150, 250, 300, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
    gen = cabi.ltg_gen_state(wp1t_bf16=0x1000, q0_last=0x2000, q0_lr_hist=0x3000, q0_ord=0, q0_period=1)
    bt = cabi.ltg_batch(n_rows=16)
    for flags, ok in ((0, True), (cabi.LTG_PIPE_TAIL_OWN | cabi.LTG_PIPE_WIDE_GRAD | cabi.LTG_PIPE_SLICE_IN_TOUCH, True), (1 << 8, False), (64, False)):
        pp = cabi.ltg_pipe(sync=0x4000, shadow_out=0x5000, flags=flags)
        assert (lib.ltg_g_step_sharded_plan(C.byref(sh), C.byref(gen), C.byref(bt), C.byref(pp)) == cabi.LTG_PLAN_SHADOW) == ok, flags
    # the forward-only tower's split weights live in the workspace only where that kernel serves the sizes (h0 <= 128, h3 <= 320, fp32 discriminator)
    wide = cabi.ltg_config(1000, 600, 200, 1000, 2048, 1024, 512, 256, 0, 0, 0, 0, 1, 1, 1e-4, 0.9, 0.999, 1e-8, 1)
    assert lib.ltg_workspace_bytes(C.byref(good), 1, 64) - lib.ltg_workspace_bytes(C.byref(cabi.ltg_config(1000, 600, 200, 1000, 100, 150, 250, 324, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)), 1, 64) > 900000
    assert lib.ltg_workspace_bytes(C.byref(wide), 1, 64) > 0
    # the one-shot exchange (ABI v14): sizing and argument checks happen on the host
    assert lib.ltg_oneshot_stage_bytes(0, 100) == 0 and lib.ltg_oneshot_stage_bytes(17, 100) == 0
    assert lib.ltg_oneshot_stage_bytes(8, 60000) == 256 + 2 * 8 * 60000 * 4 and lib.ltg_oneshot_expired_offset(8) == (2 * 8 + 2) * 4
    os_ = cabi.ltg_oneshot(2, 0, 0, 0, 100)
    buf = (C.c_float * 4)()
    assert lib.ltg_oneshot_all_reduce(None, None, 4, cabi.LTG_NCCL_FLOAT32, cabi.LTG_NCCL_SUM, C.byref(os_), None) == -1
    assert lib.ltg_oneshot_all_reduce(buf, buf, 4, cabi.LTG_NCCL_FLOAT32, cabi.LTG_NCCL_SUM, None, None) == -1
    assert lib.ltg_oneshot_all_reduce(buf, buf, 4, 0, cabi.LTG_NCCL_SUM, C.byref(os_), None) == -1               # not float32
    assert lib.ltg_oneshot_all_reduce(buf, buf, 101, cabi.LTG_NCCL_FLOAT32, cabi.LTG_NCCL_SUM, C.byref(os_), None) == -1    # beyond max_floats
    assert lib.ltg_oneshot_all_gather(buf, buf, 4, cabi.LTG_NCCL_FLOAT32, C.byref(os_), None) == -1              # stages not mapped
    assert os_.seq == 0                                                                                            # nothing was issued


def test_discriminator_layer_widths_below_one_are_refused_without_gpu():
    """A layer of width 0 (or less) has nothing to compute: LTG_EINVAL / zero sizes from every entry point before any launch, and a ValueError
    from Engine before it touches the library.  Width 1 is a valid discriminator (tests/test_gpu_parity.py holds (1, 1, 1, 1) and (4, 1, 3, 4)
    to the oracle)."""
    from ltgan import _cabi as cabi
    from ltgan.engine import Engine
    lib = cabi.load()
    mk = lambda hs: cabi.ltg_config(1000, 600, 200, 1000, *hs, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
    for hs in ((1, 1, 1, 1), (4, 1, 3, 4)):
        c = mk(hs)
        assert lib.ltg_workspace_bytes(C.byref(c), 100, 2000) > 0 and lib.ltg_d_grad_floats(C.byref(c)) > 0, hs
    for hs in ((0, 150, 250, 300), (100, 0, 250, 300), (100, 150, 0, 300), (100, 150, 250, 0), (100, -1, 250, 300)):
        c = mk(hs)
        assert lib.ltg_workspace_bytes(C.byref(c), 100, 2000) == 0 and lib.ltg_d_grad_floats(C.byref(c)) == 0, hs
        assert lib.ltg_d_step(C.byref(c), None, None, None, None, None, None, 0, None) == -1, hs
        assert lib.ltg_d_apply(C.byref(c), None, None, 1, None, None) == -1, hs
        with pytest.raises(ValueError, match="at least 1"):
            Engine(1000, h_sizes=hs, device="cpu")


def test_one_call_step_plan_is_a_pure_function_of_its_arguments():
    """ltg_g_step_sharded_plan (ABI v13) tells the host what a call will do -- catch the next batch's rows up ahead, write the second
    shadow buffer -- so that the host's bookkeeping (caught_up, the exchange of the two shadow pointers) never guesses.  Host-only: the
    pointers below are never dereferenced."""
    from ltgan import _cabi as cabi
    lib = cabi.load()
    big = cabi.ltg_config(25024, 600, 200, 25024, 100, 150, 250, 300, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
    assert big.precision == cabi.LTG_PREC_BF16
    fake = lambda k: 0x10000 * (k + 1)                       # distinct non-NULL addresses
    arr = lambda o: (cabi.vp * 8)(*[fake(o + i) for i in range(8)])
    gen = cabi.ltg_gen_state(arr(0), arr(8), arr(16), fake(30), fake(31), fake(32), 0, 32)
    bt = cabi.ltg_batch(100, 50, fake(40), fake(41), None, None, fake(42), fake(43), fake(44), fake(45), fake(46))
    assert lib.ltg_g_step_sharded_ok(C.byref(big), C.byref(gen), 100) == 1
    pipe = lambda flags=0, sync=fake(50), mark=fake(51), shadow=fake(52): cabi.ltg_pipe(fake(60), fake(61), fake(62), None, fake(63), fake(64), fake(65),
                                                                                       flags, 1, sync, None, mark, None, 0, 0, shadow)
    plan = lambda p, b=bt: lib.ltg_g_step_sharded_plan(C.byref(big), C.byref(gen), C.byref(b), C.byref(p))
    assert plan(pipe()) == cabi.LTG_PLAN_AHEAD | cabi.LTG_PLAN_SHADOW
    assert plan(pipe(mark=None)) == cabi.LTG_PLAN_SHADOW and plan(pipe(shadow=None)) == cabi.LTG_PLAN_AHEAD
    assert plan(pipe(shadow=fake(30))) == cabi.LTG_PLAN_AHEAD                  # the "second" buffer is the shadow itself: in place
    for fl in (cabi.LTG_PIPE_EVENTS, cabi.LTG_PIPE_NO_DEC1_FORK):               # no device words: neither
        assert plan(pipe(flags=fl)) == 0
    assert plan(pipe(sync=None)) == 0
    for fl in (cabi.LTG_PIPE_NO_SLICE_FORK, cabi.LTG_PIPE_SLICE_IN_TOUCH):      # the slice not on the side stream: no catch-up ahead
        assert plan(pipe(flags=fl)) == cabi.LTG_PLAN_SHADOW
    no_uitem = cabi.ltg_batch(100, 50, fake(40), fake(41), None, None, fake(42), fake(43), fake(44), fake(45), None)
    assert plan(pipe(), no_uitem) == cabi.LTG_PLAN_SHADOW
    small = cabi.ltg_config(1000, 600, 200, 1000, 100, 150, 250, 300, 0, 0, 0, 0, 1, 0, 1e-4, 0.9, 0.999, 1e-8, 1)
    assert lib.ltg_g_step_sharded_plan(C.byref(small), C.byref(gen), C.byref(bt), C.byref(pipe())) == 0    # the call itself would be refused


def test_checkpoint_rng_state_round_trips_as_plain_types():
    """format-3 model files hold tensors and plain numbers only (they load with weights_only=True): the batch-shuffle RNG state
    (train.py:285) goes through (name, int64 tensor of the 624 keys, pos, has_gauss, cached_gaussian)."""
    import io

    import numpy as np
    import torch
    from ltgan.train import _rng_state_numpy, _rng_state_plain
    r = np.random.RandomState(5)
    r.shuffle(np.arange(10))
    r.normal()                                         # leaves a cached gaussian behind
    buf = io.BytesIO()
    torch.save({"format": 3, "shuffle_rng_state": _rng_state_plain(r.get_state())}, buf)
    buf.seek(0)
    st = torch.load(buf, map_location="cpu", weights_only=True)
    r2 = np.random.RandomState(0)
    r2.set_state(_rng_state_numpy(st["shuffle_rng_state"]))
    assert np.array_equal(r.randint(0, 1 << 30, 50), r2.randint(0, 1 << 30, 50)) and r.normal() == r2.normal()


def test_product_path_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ltgan import _cabi as cabi
    from ltgan.engine import Engine
    with pytest.raises(cabi.LtgError):
        Engine(100)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "long-tail-gan_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "/root/reference" not in src, f


def test_wrapper_contract_shapes():
    """generator.py:4-22 / discriminator.py:3-58 signatures (no device work: handles only)."""
    from ltgan.generator import MultiVAE, Placeholder
    vae = MultiVAE([200, 600, 1000])
    for name, default in (("input_ph", None), ("keep_prob_ph", 0.75), ("is_training_ph", 0.0), ("anneal_ph", 1.0)):
        ph = getattr(vae, name)
        assert isinstance(ph, Placeholder) and ph.default == default
    assert vae.q_dims == [1000, 600, 200] and vae.dims == [1000, 600, 200, 600, 1000]
    with pytest.raises(NotImplementedError):
        MultiVAE([200, 600, 1000], lam=0.01)


def test_bench_rejects_gpus_launcher_mismatch():
    """`--gpus N` must agree with the launcher's WORLD_SIZE: a mismatch exits non-zero instead of measuring one GPU and
    labelling it N (checked before torch is imported, so this runs without a GPU)."""
    import subprocess, sys
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode != 0 and "WORLD_SIZE" in (out.stderr + out.stdout)


def test_bench_parent_counts_gpus_without_the_hip_runtime(monkeypatch):
    """`python bench.py --gpus N` starts its ranks from a parent that must never load the HIP runtime (a process that touched the GPU may
    not start another program on this pool): the device count comes from the visibility variables or from sysfs, not from torch."""
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    was_loaded = "torch" in sys.modules
    spec.loader.exec_module(bench)
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,1,2")
    assert bench.visible_gpus() == 3
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "5")
    assert bench.visible_gpus() == 1
    monkeypatch.delenv("HIP_VISIBLE_DEVICES")
    monkeypatch.delenv("ROCR_VISIBLE_DEVICES")
    assert bench.visible_gpus() >= 0                      # sysfs (0 in a container without a GPU)
    assert was_loaded or "torch" not in sys.modules      # importing bench.py and counting devices pulls in no torch


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_ranks_choose_their_backend_when_the_parent_could_not_count_gpus():
    """sysfs may be unreadable inside a container: the parent then forces nothing, the ranks decide from torch.cuda.device_count(),
    and a gloo fallback is recorded in the result line (config.backend_choice)."""
    bench = _bench_module()
    assert bench.choose_backend(8, 8, env={}) == ("nccl", "one GPU per rank")
    b, note = bench.choose_backend(2, 1, env={})
    assert b == "gloo" and "fallback" in note and "2 ranks on 1" in note
    b, note = bench.choose_backend(2, 1, env={"LTGAN_DIST_BACKEND": "gloo"})
    assert b == "gloo" and "LTGAN_DIST_BACKEND" in note
    assert bench.choose_backend(4, 8, env={"LTGAN_DIST_BACKEND": "nccl"})[0] == "nccl"


def test_bench_step_fraction_is_priced_on_the_bytes_the_step_moves():
    """roofline.step_frac uses the lazy clock's byte model when the clock is on (it cannot exceed 1 by construction: the model counts
    only what the step has to move); SURVEY 8/d4's dense-Adam count sits beside it under its own key and is never smaller."""
    import types
    import numpy as np
    bench = _bench_module()
    nb, B, I = 4, 100, 200000
    indptr = np.arange(0, nb * B + 1, dtype=np.int64) * 30
    idx = types.SimpleNamespace(train=types.SimpleNamespace(indptr=indptr))
    views = [dict(lo=b * B, hi=(b + 1) * B, n_real=900, n_slots=950) for b in range(nb)]
    data = types.SimpleNamespace(n_batches=nb, view=lambda b: views[b])
    for lazy in (True, False):
        eng = types.SimpleNamespace(I_global=I, H=600, Z=200, h0=100, h1=150, h2=250, h3=300, lazy_q0=lazy, q0_period=32)
        f = bench.step_fracs(idx, data, eng, 10, None, 1e-3, 1)
        assert f["step_algorithmic_bytes"] <= f["step_algorithmic_bytes_dense_adam"] and f["step_frac"] <= f["step_frac_vs_dense_adam_bytes"]
        assert (f["step_algorithmic_bytes"] < f["step_algorithmic_bytes_dense_adam"]) == lazy
        # a step that took exactly the time its bytes need at 8 TB/s sits at 1.0 on its own model
        t = f["step_algorithmic_bytes"] / bench.PEAK["hbm"]
        assert abs(bench.step_fracs(idx, data, eng, 10, None, t, 1)["step_frac"] - 1.0) < 1e-12


def test_default_initialisers_match_the_reference_distributions():
    """a3: MultiVAE.py:199-207,219-225 (Xavier-uniform weights, truncated-normal sigma = 1e-3 biases) and
    discriminator.py:14-41 (truncated-normal sigma = 0.1 matrices, zero biases): shapes, hard bounds and moments."""
    import numpy as np
    from ltgan.engine import init_discriminator_host, init_generator_host
    I, H, Z = 1000, 600, 200
    g = init_generator_host(I, H, Z, seed=98765)
    assert [a.shape for a in g] == [(I, H), (H, 2 * Z), (Z, H), (I, H), (H,), (2 * Z,), (H,), (I,)]
    for a, (fi, fo) in zip(g[:4], [(I, H), (H, 2 * Z), (Z, H), (H, I)]):
        lim = np.sqrt(6.0 / (fi + fo))
        assert np.abs(a).max() <= lim and np.abs(a).max() > 0.98 * lim                       # uniform on [-lim, lim]
        assert abs(a.mean()) < 0.02 * lim and abs(a.std() - lim / np.sqrt(3.0)) < 0.01 * lim   # std of U(-l, l) = l / sqrt(3)
    for b in g[4:]:
        assert np.abs(b).max() <= 2e-3 and abs(b.mean()) < 3e-4 and abs(b.std() - 0.88e-3) < 1.5e-4   # N(0, s) cut at 2 s: std 0.88 s
    emb, d = init_discriminator_host(1000, (100, 150, 250, 300), seed=0)
    assert emb.shape == (1000, 100) and [a.shape for a in d] == [(100, 150), (150,), (100, 250), (250,), (400, 300), (300,), (300,), (1,)]
    for a in [emb, d[0], d[2], d[4], d[6]]:
        assert np.abs(a).max() <= 0.2 and abs(a.std() - 0.088) < (0.02 if a.size < 1000 else 0.004) and abs(a.mean()) < 0.02
    for b in (d[1], d[3], d[5], d[7]):
        assert not b.any()
    g2 = init_generator_host(I, H, Z, seed=98765)
    assert all(np.array_equal(x, y) for x, y in zip(g, g2))                                  # seeded: reproducible


def test_factory_registry_and_config_ini_defaults(tmp_path, monkeypatch):
    """b2 without a device: discriminator() before generator() fails with a clear error; ./config.ini supplies the
    discriminator sizes and the learning rate of a bare generator(pro_dir) call."""
    from ltgan import generator as G
    from ltgan.discriminator import discriminator
    G.reset_default_graph()
    with pytest.raises(ValueError, match="generator"):
        discriminator(1000, 1000, 100, 150, 250, 300)
    monkeypatch.chdir(tmp_path)
    assert G._config_ini_defaults() == {}
    (tmp_path / "config.ini").write_text("[Long-Tail-GAN]\nh0_size = 64\nh1_size = 96\nh2_size = 160\nh3_size = 128\nLEARNING_RATE = 0.0003\n")
    assert G._config_ini_defaults() == {"h_sizes": (64, 96, 160, 128), "lr": 0.0003}


def test_bench_reads_the_newest_tracked_rocprof_summary_and_leaves_the_gate_kernels_out():
    """roofline.frac follows from profiles/: bench.py finds the newest r<N>_<workload>_kernel_stats.csv of a workload, adds up template
    instantiations under the kernel's base name, and neither the dominant-kernel ranking nor its percentages count the parked one-wave gates."""
    bench = _bench_module()
    rows, fn = bench.rocprof_summary("askubuntu")
    assert fn is not None and int(fn[1:fn.index("_")].rstrip("abc")) >= 6 and fn.endswith("_askubuntu_kernel_stats.csv"), fn
    assert "fk_d_bwd1" in rows and rows["fk_d_bwd1"][0] == 3960 and "k_gate_wait" in rows           # (both launches of the forked kernel in one row)
    work = {k: v for k, v in rows.items() if k not in bench.ROCPROF_NOT_WORK}
    assert max(work, key=lambda k: work[k][1]) == "fk_d_bwd1"
    for wl in ("c4", "ml20m", "custom:25024"):
        r, f = bench.rocprof_summary(wl)
        assert f is not None and "k_dec1_bwd_adam_stream" in r, wl
    assert bench.rocprof_summary("custom:777") == (None, None)
    for probe, names in bench.ROCPROF_KERNELS.items():
        assert isinstance(names, tuple) and names, probe


def test_bench_dump_outputs_writes_float32_arrays_within_budget_and_samples_the_same_rows(tmp_path):
    """--dump-outputs: every array a caller of the timed path holds goes to DIR/<name>.npy as float32; an array above the per-array cap
    keeps a fixed, seeded sample of whole rows (the same rows from run to run), and the dump stays under 64 MB."""
    import types
    import numpy as np
    import torch
    bench = _bench_module()
    g = torch.Generator().manual_seed(3)
    big = torch.randn(200000, 8, generator=g)                                  # 1.6 M values: sampled
    gen = [big, torch.randn(600, 400, generator=g), torch.randn(200, 600, generator=g), torch.randn(600, 1000, generator=g)] + \
          [torch.randn(n, generator=g) for n in (600, 400, 600, 1000)]
    disc = [torch.randn(7, 5, generator=g) for _ in range(6)] + [torch.randn(5, 1, generator=g), torch.randn(1, generator=g)]
    eng = types.SimpleNamespace(generator_params_tf=lambda: gen, discriminator_params_tf=lambda: disc)
    tr = types.SimpleNamespace(d_losses=torch.randn(10, 8, generator=g), g_losses=torch.randn(10, 8, generator=g))
    data = types.SimpleNamespace(fake_cnt=torch.arange(101, dtype=torch.int32), fake_gen=torch.arange(3000000, dtype=torch.int32),
                                 fake_pop=torch.full((5,), -1, dtype=torch.int32))
    bench.dump_outputs(str(tmp_path / "a"), tr, eng, data)
    bench.dump_outputs(str(tmp_path / "b"), tr, eng, data)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(["d_losses.npy", "g_losses.npy", "fake_cnt.npy", "fake_gen.npy", "fake_pop.npy"] +
                           ["gen_%s.npy" % n for n in ("W_q0", "W_q1", "W_p0", "W_p1", "b_q0", "b_q1", "b_p0", "b_p1")] +
                           ["disc_%d.npy" % i for i in range(8)])
    total = 0
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and x.size <= bench.DUMP_MAX_VALUES and np.array_equal(x, y), f
        total += x.nbytes
    assert total <= 64 << 20
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "gen_W_q1.npy"), gen[1].numpy())              # small arrays: whole, unchanged
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "fake_pop.npy"), -np.ones(5, np.float32))
    w = np.load(tmp_path / "a" / "gen_W_q0.npy")                               # sampled: whole rows of the original, in row order
    assert w.shape == (bench.DUMP_MAX_VALUES // 8, 8)
    rows = {tuple(r) for r in big.numpy()}
    assert all(tuple(r) in rows for r in w[:50])
    f = np.load(tmp_path / "a" / "fake_gen.npy")
    assert f.shape == (bench.DUMP_MAX_VALUES, 1) and np.all(np.diff(f[:, 0]) > 0) and f.max() < 3000000
