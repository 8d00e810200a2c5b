"""tests/serving_harness.py without a GPU: the port table, the arrays of the exact-sum model the seven sharded-recommender workers build
on (pinned, so that the workers keep the data their assertions depend on: a floor that binds, anchors that span two slabs, ...), and the
claim that makes that model worth having -- its encoder sum is exact in fp32 in any slab order."""
import hashlib
import itertools
import os

import numpy as np

import serving_harness as H

I, HID, N_EV = 1001, 600, 230                            # the workers' arguments and the default p_dims[1]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_every_launch_site_has_its_own_port_and_its_worker_exists():
    ports = [port for _, port in H.PORTS.values()]
    assert len(set(ports)) == len(ports) and all(1024 < p < 65536 for p in ports)
    workers = {script for script, _ in H.PORTS.values() if script.endswith("_worker.py")}
    assert len(workers) >= 16
    for script, _ in H.PORTS.values():
        assert os.path.exists(os.path.join(H.TESTS if script in workers else H.PKG, script)), script


def test_exact_sum_arrays_are_the_workers_arrays():
    """the digests of what the workers drew before they shared this function: their own lines (default_rng(3): bias, W_q0, 16 fold-in
    items per user, sorted CSR) run on a CPU with I = 1001, H = 600, n_ev = 230, and of the NEXT draw, which the workers' labels are"""
    rng = np.random.default_rng(3)
    bias, wq0, fold = H.exact_sum_arrays(rng, I, HID, N_EV)
    assert (bias.dtype, wq0.dtype, fold.indptr.dtype, fold.indices.dtype) == (np.float32, np.float32, np.int32, np.int32)
    assert bias.shape == (I,) and wq0.shape == (I, HID) and fold.shape == (N_EV, I) and fold.has_sorted_indices
    assert _sha(bias) == "3ae7d2b7e1c6b44db214113bb93278c1cf5f332f254c865bf6bbbafbc26a5cf9"
    assert _sha(wq0) == "c8675742885150966fe19274ab5618dbe4fe6b757d7043fac19bf9c680e22965"
    assert _sha(fold.indptr) == "d1e77ab3d0f5ad78659dd2f911b78d8fc32f70dbf7eb08b9e347221a15da1047"
    assert _sha(fold.indices) == "7e061c8b47af1c851524dbad10097025fbd51199086e5bc41fcf603fcb72376e"
    assert _sha(rng.integers(0, 3, I)) == "3b3252275422bdcd9c9bba7fddfb91e10f136a63a8b3afcdc1711e5605bffb0f"      # the generator's state


def test_the_encoder_sum_of_the_exact_sum_model_is_exact_in_any_slab_order():
    """per slab the fp32 sum of a user's fold-in rows of W_q0 that fall into it, the slabs' partial sums added in fp32 in every order:
    bit for bit the fp32 sum over all 16 rows, at world sizes 2, 3 and 4 with item_slab's cuts of 1 001 items"""
    from ltgan.sharded import item_slab
    bias, wq0, fold = H.exact_sum_arrays(np.random.default_rng(3), I, HID, N_EV)
    assert (np.diff(fold.indptr) == 16).all() and np.array_equal(wq0 * 64, np.round(wq0 * 64)) and np.abs(wq0).max() <= 1.0
    rows = fold.indices.reshape(N_EV, 16)
    whole = np.zeros((N_EV, HID), np.float32)
    for j in range(16):                                  # sequential fp32 adds, in the CSR's order
        whole += wq0[rows[:, j]]
    for world in (2, 3, 4):
        parts = []
        for lo, hi in (item_slab(I, r, world) for r in range(world)):
            part = np.zeros((N_EV, HID), np.float32)
            for j in range(16):
                inside = (rows[:, j] >= lo) & (rows[:, j] < hi)
                part[inside] += wq0[rows[inside, j]]
            parts.append(part)
        assert sum(int((p != 0).any()) for p in parts) == world
        for order in itertools.permutations(range(world)):
            total = np.zeros((N_EV, HID), np.float32)
            for r in order:
                total += parts[r]
            assert np.array_equal(total.view(np.uint32), whole.view(np.uint32)), (world, order)
