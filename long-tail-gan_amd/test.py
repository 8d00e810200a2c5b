#!/usr/bin/env python3
"""Test CLI with the reference's surface (Codes/test.py:30-203):

    cd <dir holding config.ini> && python <repo>/long-tail-gan_amd/test.py <dataset_dir> <checkpoint>

restores a checkpoint written by train.py (`model_<epoch>.pt`), scores `test_tr.csv` / `test_te.csv` in chunks of
20 000 users (test.py:76) with the generator forward (dropout ON: Q3), masks the fold-in items to -inf (test.py:149)
and prints `NDCG@100 \\t Recall@20 \\t Recall@50` (test.py:173).  Scores never leave the GPU (ltg_rank_metrics).
Under `python -m torch.distributed.run --nproc-per-node N` the items are sharded like in train.py.
"""
from __future__ import annotations

import os
import sys

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ltgan  # noqa: F401  (alias of this package directory)
    from ltgan import data_processing as dp
    from ltgan.dataset import EvalData
    from ltgan.discriminator import discriminator
    from ltgan.serving import Evaluator, ShardedEvaluator, _Counters, close_model, open_model  # noqa: F401
    from ltgan.train import read_config
else:
    from . import data_processing as dp
    from .dataset import EvalData
    from .discriminator import discriminator
    from .serving import Evaluator, ShardedEvaluator, _Counters, close_model, open_model  # noqa: F401
    from .train import read_config


def test_GAN(h0_size, h1_size, h2_size, h3_size, NUM_EPOCH, NUM_SUB_EPOCHS, BATCH_SIZE, DISPLAY_ITER, LEARNING_RATE, to_restore,
             model_name, dataset, GANLAMBDA, output_path, precision="bf16", device=None, batch_size_test=20000):
    """Codes/test.py:30-173 (same argument list)."""
    eng, lo, hi, rank, world, print = open_model(dataset, output_path, (h0_size, h1_size, h2_size, h3_size), LEARNING_RATE, precision, device)  # noqa: A001
    DATA_DIR = dataset + "/"
    n_items = eng.I_global
    discriminator(n_items, n_items, h0_size, h1_size, h2_size, h3_size)   # the reference's six arguments (train.py:136)
    print("Loading Test Matrix...", end="")
    tr, te, _ = dp.load_tr_te_data(os.path.join(DATA_DIR, "test_tr.csv"), os.path.join(DATA_DIR, "test_te.csv"), n_items)
    print("N_test:", tr.shape[0])
    print("Model Loaded")
    if world > 1:
        ev = ShardedEvaluator(eng, EvalData(tr, te, eng.device, item_lo=lo, item_hi=hi), chunk=batch_size_test)
    else:
        ev = Evaluator(eng, EvalData(tr, te, eng.device), chunk=batch_size_test)
    m = ev.run(rng_step=2 * 10 ** 9)
    print(str(m["ndcg"]) + "\t" + str(m["recall20"]) + "\t" + str(m["recall50"]))
    close_model(world)
    return m


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit("usage: test.py <dataset_dir> <checkpoint>   (config.ini is read from the current directory)")
    test_GAN(dataset=sys.argv[1], output_path=sys.argv[2], **read_config())
