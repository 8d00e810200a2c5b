"""Cases, inputs and bounds of the quantised-discriminator tests (ltg_config.d_precision = bf16 / fp8): tests/test_gpu_quantised_disc.py
holds the kernels to them, tests/test_quantised_disc_cpu.py the oracle at float32.

The bounds come from a NOISE MODEL, not from a device figure.  Device and fp64 oracle feed identical quantised weights and embeddings; they
differ where a GEMM result, formed with the pipe's own accumulation error, is quantised AGAIN (A1 at scale act, dpre3 at g3, dpre1 at g1): a
value near a rounding boundary then flips by a whole quantisation step (6 % in e4m3).  O.d_tower / O.d_tower_backward(jitter = (rng, rel))
multiply every quantised GEMM's result by 1 + rel N(0, 1), rel = the accumulation bound test_gemm_block_operand_modes asserts for the mode
(REL).  The FLOOR of a case is the worst over DRAWS draws of max |y_jitter - y|, of the median of the same and, for gradients, of the
per-tensor distance in the energy norm; the bound on the device is FACTOR = 4 x the floor, for the maximum and the median separately (the
worst of a few thousand heavy-tailed flip events moves about 2 x from draw to draw, and the device's error is not Gaussian; a wrong tile,
mask offset, scale or K block moves y by O(0.1)).  The median bound catches a small systematic bias that a max bound hides."""
from __future__ import annotations

import numpy as np

import helpers as Hh
from oracle import ltg_oracle as O

SEED = Hh.HOT_SEED
REL = {"bf16": 3e-6, "fp8": 1e-4}
DRAWS, FACTOR = 3, 4.0
KEEP = 0.7

# forward-only tower: (layer sizes, segment lengths).  config.ini's sizes with ragged 64-row tiles either side of a tile edge; BASELINE
# config 5's (fk8s_d_*); fk8_d_* (h0 % 128 = 64); on-the-fly mode-2 kernels (h3 % 64 != 0); staged, h3 > 512; scalar loaders; the smallest
TOWER_CASES = [((100, 150, 250, 300), (1, 63, 64, 65, 700)), ((2048, 1024, 512, 256), (1, 257)), ((192, 64, 128, 128), (5, 130)),
               ((256, 128, 128, 100), (129,)), ((512, 256, 256, 640), (257,)), ((99, 151, 250, 301), (1, 257)), ((12, 20, 28, 16), (5, 130))]
TOWER_HOT = TOWER_CASES[:2]


def case_id(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def m_tol(dq, hs):
    """the project's first-moment bound of the mode and size class (test_d_step_precision_modes); second moments: twice it"""
    if dq == "bf16":
        return 2e-3
    return 6e-2 if hs[0] >= 512 or hs[3] > 512 else 2e-2


def _biased(D, rng):
    for k in ("b1", "b2", "b3", "b4"):
        D[k] = rng.normal(0, 0.05, D[k].shape).astype(np.float32)
    return D


def _ids(rng, n, I, holes):
    pop, nic = rng.integers(0, I, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
    hole = rng.random(n) < holes
    hole[:1] = False                     # (a one-row batch keeps its row)
    pop[hole] = -1
    nic[hole] = -1
    return pop, nic


# ---------------------------------------------------------------------------------------------------------------- forward-only tower
def tower_case(hs, segs, hot=False, emb_scale=1.0, I=400):
    rng = np.random.default_rng(sum(segs) + hs[0])
    D = _biased(O.init_discriminator(I, *hs, seed=11), rng)
    if hot:
        D = Hh.hot_discriminator(D)
    if emb_scale != 1.0:
        D["emb"] = D["emb"] * np.float32(emb_scale)
    n = sum(segs)
    pop, nic = _ids(rng, n, I, 0.04)
    return dict(hs=hs, segs=segs, D=D, n=n, pop=pop, nic=nic, row0=np.concatenate([[0], np.cumsum(segs)[:-1]]).astype(np.int32),
                seg_of=np.repeat(np.arange(len(segs), dtype=np.int32), segs), steps=(1000 + 7 * np.arange(len(segs))).astype(np.int64))


def tower_oracle(c, mode, keep=KEEP, dtype=np.float64, jitter=None, steps=None):
    """y of every slot (0 at a hole), segment by segment with the segment's own dropout counter; valid [n]"""
    y = np.zeros(c["n"], np.float64)
    valid = c["pop"] >= 0
    for sidx, (r0, ns) in enumerate(zip(c["row0"], c["segs"])):
        sl = slice(r0, r0 + ns)
        dm = Hh.d_masks(SEED, int((c["steps"] if steps is None else steps)[sidx]), ns, c["hs"][1:], keep)
        v = valid[sl]
        T = O.d_tower(c["D"], np.where(v, c["pop"][sl], 0), np.where(v, c["nic"][sl], 0), dm, keep, dtype=dtype, dq=mode, jitter=jitter)
        y[sl] = np.where(v, T["y"], 0.0)
    return y, valid


def y_figures(y_got, y_want, valid):
    d = np.abs(np.asarray(y_got, np.float64) - y_want)[valid]
    return float(d.max()), float(np.median(d))


def tower_floor(c, mode, y, valid, keep=KEEP):
    """(floor of max |dy|, floor of median |dy|): the worst of DRAWS jitter draws"""
    fmax = fmed = 0.0
    for k in range(DRAWS):
        yj, _ = tower_oracle(c, mode, keep, jitter=(np.random.default_rng(7000 + k), REL[mode]))
        a, b = y_figures(yj, y, valid)
        fmax, fmed = max(fmax, a), max(fmed, b)
    return fmax, fmed


# ---------------------------------------------------------------------------------------------------------------- D step
def d_case(nr, nf, hs, hot=False, I=500):
    """a pair batch of nr real | nf fake rows, 5 % holes, non-zero biases (the inputs of test_gpu_parity._d_step_case, every bias drawn)"""
    rng = np.random.default_rng(nr * 7 + nf)
    D = _biased(O.init_discriminator(I, *hs, seed=3), rng)
    if hot:
        D = Hh.hot_discriminator(D)
    rp, rn = _ids(rng, nr, I, 0.05)
    fp, fn = _ids(rng, nf, I, 0.05)
    return dict(hs=hs, D=D, I=I, nr=nr, nf=nf, rp=rp, rn=rn, fp=fp, fn=fn, step=21, keep=KEEP)


def d_oracle(c, mode, jitter=None, parts=False):
    """(d_loss, gradients, y real | fake, valid real | fake) of the quantised pipeline in fp64; holes: id 0 with ds = 0, as _d_step_case"""
    nr, hs, keep, D = c["nr"], c["hs"], c["keep"], c["D"]
    dm = Hh.d_masks(SEED, c["step"], nr + c["nf"], hs[1:], keep)
    mr, mf = [m[:nr] for m in dm], [m[nr:] for m in dm]
    vr, vf = c["rp"] >= 0, c["fp"] >= 0
    Tr = O.d_tower(D, np.where(vr, c["rp"], 0), np.where(vr, c["rn"], 0), mr, keep, dq=mode, jitter=jitter)
    Tf = O.d_tower(D, np.where(vf, c["fp"], 0), np.where(vf, c["fn"], 0), mf, keep, dq=mode, jitter=jitter)
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = -np.where(vr, np.log(Tr["y"]), 0.0).sum() - np.where(vf, np.log(1 - Tf["y"]), 0.0).sum()
    dsr, dsf = -(1 - Tr["y"]) * vr, Tf["y"] * vf
    gr = O.d_tower_backward(D, Tr, mr, keep, dsr, dq=mode, jitter=jitter)
    gf = O.d_tower_backward(D, Tf, mf, keep, dsf, dq=mode, jitter=jitter)
    g = {k: (gr[k] + gf[k]).reshape(np.asarray(D[k]).shape) for k in gr}
    out = (float(loss), g, np.concatenate([Tr["y"], Tf["y"]]), np.concatenate([vr, vf]))
    return out + (((Tr, mr, dsr), (Tf, mf, dsf)),) if parts else out


def energy(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def d_floor(c, mode, g):
    """per tensor (energy-norm floor, max-norm floor) of the GRADIENT (a first Adam step's m is 0.1 g: the same relative figures; v =
    0.001 g^2: twice them), the worst of DRAWS jitter draws"""
    fl = {k: [0.0, 0.0] for k in O.D_KEYS}
    for d in range(DRAWS):
        gj = d_oracle(c, mode, jitter=(np.random.default_rng(7000 + d), REL[mode]))[1]
        for k in O.D_KEYS:
            fl[k][0] = max(fl[k][0], energy(gj[k], g[k]))
            fl[k][1] = max(fl[k][1], Hh.rel_err(gj[k], g[k]))
    return fl


def scaled_operands(c, parts):
    """the fp8 mode's operands times their static scales, as the oracle forms them BEFORE the e4m3 conversion: {class: [arrays]} (emb, w,
    act, g3, g1) -- for the statements about the clamp (448) and the subnormal step (2^-9) of a case"""
    D, keep, h1 = c["D"], c["keep"], c["hs"][1]
    q = lambda x, cls: O._dq(np.asarray(x, np.float64), "fp8", cls)
    ops = {"emb": [], "w": [np.asarray(D[k], np.float64) for k in ("w1", "w2", "w3")], "act": [], "g3": [], "g1": []}
    for T, m, ds in parts:
        ops["emb"] += [T["ea"], T["eb"]]
        ops["act"].append(T["hin"])
        dpC = (np.asarray(ds, np.float64)[:, None] @ np.asarray(D["w4"], np.float64).T * m[2] / keep * (1 - T["tC"] ** 2)).astype(np.float32).astype(np.float64)
        ops["g3"].append(dpC)
        dhin = q(dpC, "g3") @ q(D["w3"], "w").T
        fA, fB = (O.bf16_round((mm / keep * (1 - t ** 2)).astype(np.float32)).astype(np.float64) for mm, t in ((m[0], T["tA"]), (m[1], T["tB"])))
        ops["g1"] += [(dhin[:, :h1] * fA).astype(np.float32).astype(np.float64), (dhin[:, h1:] * fB).astype(np.float32).astype(np.float64)]
    return {k: [a * float(1 << O.FP8_S[k]) for a in v] for k, v in ops.items()}


# ---------------------------------------------------------------------------------------------------------------- e4m3 bytes
def e4m3_table():
    """value of every OCP e4m3 byte (bias 7, subnormals m / 8 * 2^-6, 0x7f / 0xff = NaN)"""
    b = np.arange(256)
    e, m = (b >> 3) & 15, (b & 7).astype(np.float64)
    v = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1.0 + m / 8.0) * np.exp2(e.astype(np.float64) - 7.0))
    v = np.where((b & 0x7F) == 0x7F, np.nan, v)
    return np.where(b & 0x80, -v, v)
