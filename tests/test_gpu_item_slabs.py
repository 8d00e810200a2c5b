"""The item-sharded path against the CPU oracle, in ONE process: every rank of a run is an engine of its own over its item slab
(helpers.SlabRig), and the exchanges between them are sums and concatenations in rank order on the device -- no rank launches, no
torch.distributed.  What is held to the oracle here is the arithmetic of the slab code (the dropout key item_lo + it, the range tests on
f_gen - item_lo and cand_idx - item_lo, the rank-term combine, row_norm2 of the full row on a partial row); the multi-rank tests
(test_gpu_sharded.py) remain the check of the transports.

  cut-point G step   helpers.SLAB_G through test_gpu_parity._g_step_case(ranks = R, path = "cut-points"): one oracle on the full I, the
                     model the ranks hold together at the unsharded bounds, replicas equal bit for bit
  one-call G step    every rank of the streaming cases again through ltg_g_step_sharded, its peers replayed from the cut-point run's record
  slab forward       ltg_g_fwd_enc / ltg_g_fwd_rest / ltg_rowstats_combine at test_forward_parity's bounds, one batch and a span of batches
  sampler            ltg_gather_cand_logits + ltg_sample_pairs from cand_logit, exactly the unsharded call's pairs"""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as Hh
import test_gpu_parity as TP
from oracle import ltg_oracle as O

pytestmark = pytest.mark.gpu

SEED = TP.SEED


def _slab_id(case):
    p, I, B, R, history, warm = case
    return "%s-%d-%d-r%d%s%s" % (p, I, B, R, TP._history_id(history), "-warm" if warm else "")


@functools.lru_cache(maxsize=None)
def _cut_point_run(case):
    """(the case with its oracle, what the ranks left, the rig with its record) of a SLAB_G case: computed once, shared by the cut-point test
    and the one-call test of the case, and left unchanged by both.  The oracle assertions run inside."""
    p, I, B, R, history, warm = case
    return TP._g_step_case(p, I, B, "cut-points", warm, history=history, ranks=R)


@pytest.mark.parametrize("case", Hh.SLAB_G, ids=_slab_id)
def test_cut_point_g_step_over_item_slabs_matches_oracle(case):
    """ShardedTrainer._g_one's cut-point sequence (ltg_g_fwd_enc, ltg_g_fwd_rest, ltg_g_bwd_dec, ltg_g_bwd_dec1, ltg_g_bwd_rest, ltg_g_flush) on
    R slab engines in lock step, the three exchanges summed by hand in rank order.  W_q0 / W_p1t / b_p1 and their moments concatenated over
    the ranks, everything else from rank 0 -- after every rank's copy proved equal to rank 0's bit for bit (SlabRig.assemble) -- against the
    oracle's ONE update on the full I: test_g_step_parity's bounds (m 5e-4 fp32 / 2e-3 bf16, v twice that, the Adam move, the losses; from
    warm moments _check_warm_adam).  History and fake pairs sit on item 0, I - 1 and either side of every cut; row 5 has nothing in the last
    slab.  8 200 items over two ranks: slabs of 4 160 and 4 040 items take different routes (tests/test_routes_cpu.py)."""
    _, I, _, R, _, _ = case
    c, _, rig = _cut_point_run(case)
    assert [(e.item_lo, e.item_hi) for e, _, _, _ in rig.ranks] == Hh.slab_cuts(I, R) and rig.record is not None
    assert all(e.adam_t == c.t0 + 1 for e, _, _, _ in rig.ranks)


class ReplayComm:
    """ltg_comm of rank `rank` of R whose peers are a recording (SlabRig.record): the all-reduce keeps what the rank contributed and puts the
    recorded total in its place, the all-gather keeps the send block, copies it to block `rank` and fills the other blocks from the
    recording.  Device-to-device copies on the current stream only; no synchronisation, and nothing is raised through the C frame (2 on
    any error, as _rccl.HostComm).  A test rig, not a transport."""

    def __init__(self, pipe, R, rank, record):
        from ltgan import _cabi as cabi
        self.R, self.rank, self.record = R, rank, record
        self.bufs = {"h1": pipe.h1pre, "rowpart": pipe.rowpart_all, "dh2": pipe.dh2}
        self.sent = {}
        self.errors = []
        self._cabi = cabi
        self._ar = cabi.ALL_REDUCE_FN(self._all_reduce)              # (kept alive with the object)
        self._ag = cabi.ALL_GATHER_FN(self._all_gather)
        self.c = cabi.ltg_comm(None, R, rank, C.cast(self._ar, C.c_void_p), C.cast(self._ag, C.c_void_p))

    def _find(self, ptr, count):
        for name, t in self.bufs.items():
            base = t.data_ptr()
            if base <= ptr and ptr + 4 * count <= base + 4 * t.numel():
                return name, t.view(-1)[(ptr - base) // 4:(ptr - base) // 4 + count]
        raise KeyError("pointer %x is not inside an exchange buffer of the pipe" % ptr)

    def _all_reduce(self, send, recv, count, dtype, op, comm, stream):
        try:
            if dtype != self._cabi.LTG_NCCL_FLOAT32 or op != self._cabi.LTG_NCCL_SUM or send != recv:
                return 1
            name, t = self._find(recv, count)
            total = self.record[name + "_all"].view(-1)
            if name == "rowpart" or name in self.sent or total.numel() != count:
                return 1
            self.sent[name] = t.clone()
            t.copy_(total)
            return 0
        except Exception as e:                                       # an exception must not unwind through the C frame
            self.errors.append(repr(e))
            return 2

    def _all_gather(self, send, recv, sendcount, dtype, comm, stream):
        try:
            if dtype != self._cabi.LTG_NCCL_FLOAT32:
                return 1
            _, src = self._find(send, sendcount)
            name, out = self._find(recv, self.R * sendcount)
            if name != "rowpart" or name in self.sent or self.record["rowpart"][0].numel() != sendcount:
                return 1
            self.sent[name] = src.clone()
            for q in range(self.R):
                out[q * sendcount:(q + 1) * sendcount].copy_(self.sent[name] if q == self.rank else self.record["rowpart"][q])
            return 0
        except Exception as e:
            self.errors.append(repr(e))
            return 2


ONE_CALL = [c for c in Hh.SLAB_G if min(hi - lo for lo, hi in Hh.slab_cuts(c[1], c[3])) >= 8192]


@pytest.mark.parametrize("case", ONE_CALL, ids=_slab_id)
def test_one_call_g_step_with_replayed_peers_equals_the_cut_point_step(case):
    """include/ltg.h: ltg_g_step_sharded "equals ... the cut-point sequence's [results] bit for bit".  Every rank of the streaming cases runs
    the one-call step from the same start state on a fresh slab engine, with a communicator that replays its peers from the cut-point
    run's record: what the rank hands to each of the three exchanges, and after ltg_g_flush every tensor, moment and the loss, equal the
    cut-point rank's bit for bit; the assembled model passes the oracle assertions at the same bounds."""
    import torch
    from ltgan.engine import Pipe
    _, _, B, R, _, _ = case
    c, cut_got, rig = _cut_point_run(case)
    rec = rig.record
    engines, losses = [], []
    for r in range(R):
        eng, dd, batch, acts = rig.rank(r)
        ref = rig.ranks[r][0]
        assert eng.sharded_step_ok(B) and eng.g_route(B).sharded_ok == 1
        pipe = Pipe(eng, B, R)
        comm = ReplayComm(pipe, R, r, rec)
        fake, cnt_t = TP._g_fake(c, eng.device)
        go = eng.g_opts(cnt_t, TP.G_ANNEAL, TP.G_LAM, TP.G_KEEP, 1.0, TP.G_DKEEP, TP.G_STEP, TP.G_DSTEP)
        loss = torch.zeros(8, dtype=torch.float32, device=eng.device)
        eng.g_step_sharded(batch, fake, acts, go, pipe, comm, loss_out=loss)
        eng.g_flush()
        torch.cuda.synchronize()
        assert not comm.errors, comm.errors
        assert pipe.expired_waits() == 0
        for name in ("h1", "rowpart", "dh2"):
            assert name in comm.sent, (r, name, "never exchanged")
            want = rec[name][r].reshape(-1)
            assert torch.equal(comm.sent[name], want), (r, name, float((comm.sent[name] - want).abs().max()))
        for i in range(8):
            for what, a, b in (("p", eng.g_p[i], ref.g_p[i]), ("m", eng.g_m[i], ref.g_m[i]), ("v", eng.g_v[i], ref.g_v[i])):
                assert torch.equal(a, b), (r, what, i, float((a - b).abs().max()))
        engines.append(eng)
        losses.append(loss)
    for r in range(R):
        assert np.array_equal(losses[r][:6].cpu().numpy(), cut_got[0][:6]), (r, "loss")      # (every cut-point rank's: SlabRig.assemble)
    p_got, m_got, v_got, loss = Hh.SlabRig.assemble(engines, losses)
    TP._g_assert(c, (loss, p_got, m_got, v_got), "one-call", tag=_slab_id(case))


# ---- slab forward (phase C / serving._slab_forward): (I, B, R)
FWD_SLABS = [(I, B, R, p) for I, B, R in ((1000, 100, 2), (1101, 37, 9), (16520, 100, 2)) for p in ("fp32", "bf16")]
FWD_STEP, FWD_KEEP = 7, 0.75


def _slab_forward(X_all, B, b, R, precision, P, fopts):
    """(h1, h2, logits over all items, lse) of the slab forward of batch (or span) b: every rank's h1 / h2 / lse equal rank 0's bit for bit"""
    import torch
    I = X_all.shape[1]
    rig = Hh.SlabRig(X_all, B, b, R, lambda lo, hi: TP._engine(I, precision, item_lo=lo, item_hi=hi), Hh.gen_to_engine(P))
    n = rig.ranks[0][2].n_rows
    _, _, _, rp_all = rig.forward(fopts)
    for eng, _, _, acts in rig.ranks:
        acts.lse.fill_(float("nan"))
        eng.rowstats_combine(rp_all, R, n, acts.lse)
    torch.cuda.synchronize()
    a0 = rig.ranks[0][3]
    for r, (_, _, _, acts) in enumerate(rig.ranks[1:], 1):
        for k in ("h1", "h2", "lse"):
            assert torch.equal(getattr(acts, k)[:n], getattr(a0, k)[:n]), ("replica", k, r)
    logits = torch.cat([acts.logits[:n] for _, _, _, acts in rig.ranks], dim=1)
    return a0.h1[:n].cpu().numpy(), a0.h2[:n].cpu().numpy(), logits.cpu().numpy(), a0.lse[:n].cpu().numpy()


def _two_batches(I, B, R, seed):
    """(X_all of two uniform batches, batch 1, P): row 2 of batch 1 holds the slab edges"""
    import scipy.sparse as sp
    rng, X, P = TP._problem(I, B, seed=seed)
    X_all = sp.vstack([Hh.random_history(np.random.default_rng(seed + 1), B, I), X]).tocsr()
    X_all = Hh.with_edge_history(X_all, B + 2, Hh.slab_edges(Hh.slab_cuts(I, R)))
    return X_all, X_all[B:2 * B].tocsr(), P


@pytest.mark.parametrize("I,B,R,precision", FWD_SLABS, ids=["%d-%d-r%d-%s" % c for c in FWD_SLABS])
def test_slab_forward_matches_oracle(I, B, R, precision):
    """ltg_g_fwd_enc on every slab, h1 summed in rank order, ltg_g_fwd_rest without fake pairs, ltg_rowstats_combine on the gathered partials:
    h1, h2, the concatenated logits and the lse of the full rows at test_forward_parity's bounds"""
    tol = 2e-4 if precision == "fp32" else 1e-3
    X_all, X, P = _two_batches(I, B, R, I + B)
    h1, h2, logits, lse = _slab_forward(X_all, B, 1, R, precision, P, lambda eng: eng.fwd_opts(FWD_KEEP, 1.0, FWD_STEP))
    mask = Hh.dropout_mask_dense(SEED, FWD_STEP, B, I, FWD_KEEP)
    F = O.vae_forward(P, X.toarray(), mask, FWD_KEEP, Hh.eps_dense(SEED, FWD_STEP, B, 200), 1.0, 1.0, np.float64, quant=(precision == "bf16"))
    print("slab forward I=%d B=%d R=%d %s: h1 %.2e h2 %.2e logits %.2e lse %.2e" % (I, B, R, precision, Hh.rel_err(h1, F["h1"]), Hh.rel_err(h2, F["h2"]),
                                                                                   Hh.rel_err(logits, F["logits"]), np.abs(lse - F["lse"]).max()))
    assert Hh.rel_err(h1, F["h1"]) < 2e-5
    assert Hh.rel_err(h2, F["h2"]) < 1e-4
    assert Hh.rel_err(logits, F["logits"]) < tol
    assert np.abs(lse - F["lse"]).max() < tol


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_slab_forward_over_a_span_of_batches_matches_oracle(precision):
    """the form Trainer.create_phase and serving._slab_forward use: is_training = 0 and rows_per_step over a span of (100, 100, 50) rows at
    1 000 items on two slabs -- batch k draws its dropout with counter step + k and its local rows, on every slab alike"""
    I, R, rows, step = 1000, 2, (100, 100, 50), 21
    tol = 2e-4 if precision == "fp32" else 1e-3
    rng, X, P = TP._problem(I, sum(rows), seed=3 * I + sum(rows))
    X = Hh.with_edge_history(X, 102, Hh.slab_edges(Hh.slab_cuts(I, R)))

    def fopts(eng):
        fo = eng.fwd_opts(FWD_KEEP, 0.0, step)
        fo.rows_per_step = rows[0]
        return fo
    h1, h2, logits, lse = _slab_forward(X, rows[0], (0, len(rows)), R, precision, P, fopts)
    assert h1.shape[0] == sum(rows)
    r0 = 0
    for k, n in enumerate(rows):
        mask = Hh.dropout_mask_dense(SEED, step + k, n, I, FWD_KEEP)
        F = O.vae_forward(P, X[r0:r0 + n].toarray(), mask, FWD_KEEP, np.zeros((n, 200)), 0.0, 1.0, np.float64, quant=(precision == "bf16"))
        sl = slice(r0, r0 + n)
        assert Hh.rel_err(h1[sl], F["h1"]) < 2e-5, k
        assert Hh.rel_err(h2[sl], F["h2"]) < 1e-4, k
        assert Hh.rel_err(logits[sl], F["logits"]) < tol, k
        assert np.abs(lse[sl] - F["lse"]).max() < tol, k
        r0 += n


# ---- phase C's sampler over slabs: (I, B, R, with_zero_probs, rows_per_step)
SAMPLER_SLABS = [(1000, 100, 2, False, 0), (1000, 100, 2, True, 0), (1101, 37, 9, False, 0), (1101, 37, 9, True, 0), (1000, 100, 2, False, 50)]


@pytest.mark.parametrize("I,B,R,with_zero_probs,rows_per_step", SAMPLER_SLABS, ids=["%d-%d-r%d-%s-%d" % c for c in SAMPLER_SLABS])
def test_sampler_over_item_slabs_equals_the_unsharded_call(I, B, R, with_zero_probs, rows_per_step):
    """test_gpu_parity._sampler_case with the ranks' cuts: candidates on either side of every cut, on item 0 and on item I - 1; the added
    gather buffers equal logits[b, cand] exactly, ltg_sample_pairs from cand_logit returns the unsharded call's gen / pop / cnt on the
    first and on the last rank, and the unsharded call passes the oracle comparison (at most one legal flip)"""
    rng = np.random.default_rng(9 + I + with_zero_probs + rows_per_step)
    TP._sampler_case(rng, I, B, TP._sampler_problem(rng, B, I, with_zero_probs), with_zero_probs, cuts=Hh.slab_cuts(I, R), rows_per_step=rows_per_step)
