"""The serving layer's one source of catalogue-wide lists (serving.SlabLists) and its one chunk walk (Recommender.run, shared by
ShardedRecommender) without a GPU: a fake engine on CPU tensors records every call (tests/serving_cpu_worker.py).  Every gathered and
merged list must equal torch.topk on the full 150-column logits on both ranks of a world-size-2 gloo run -- slabs of 128 and 22 items, a
full chunk of 5 rows and a short last one of 3, lists of 7 and of 4 entries alternating on one set of buffers -- and the recorded
sequence of engine calls and collectives must be the one written out in the worker for plain, ruled (two reserved groups, and none),
diversified, calibrated, capped, floored (both by log-probability and by the logit) and share-targeted lists and for the audiences (beside
the lists and alone, k = 0), each without and with a report and / or explanations -- for the rules over the whole split the second pass
after the match --, item-sharded and not; the full-row lse is combined exactly where something ranks by log-probability.  No two rules
go together, and k = 0 goes with nothing that needs lists."""
from serving_harness import run_ranks


def test_unsharded_lists_are_written_directly_and_the_calls_are_the_direct_ones():
    import serving_cpu_worker as W
    W.unsharded()


def test_world_size_two_lists_and_call_sequences():
    run_ranks("serving_cpu_worker.py", [], 2, "SERVING_CPU_OK", limit=600, env={"OMP_NUM_THREADS": "1"})

