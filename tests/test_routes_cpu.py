"""The kernel route of every shape the GPU tables claim something about (include/ltg.h: ltg_g_route / ltg_d_route; host-only, no GPU).

The GPU tests name the route a shape is meant to reach in comments -- "small slab", "first streaming form, ragged tail", "d_wide: l1 / bwd1
64, l2 -32, bwd2 128 tiles".  This module holds the library to those statements: it imports the tables themselves (helpers.HOT_FWD / HOT_G / SLAB_G -- every rank's slab of the last --,
test_gpu_parity.G_CASES / G_SKEWED / WARM_CASES / D_SIZES / D_STEP_CASES, test_gpu_quantised_disc.D_Q), and every case of them has to have
its route written down here.  If a threshold moves, a case no longer exercises the kernel its comment names, and this fails before any GPU
run.  The expected values are written out from the selection rules of csrc/ltg_kernels.hip as they stood before the routes existed (and
were checked against a kernel trace of that build), not computed by a second copy of the rules."""
import ctypes as C

import pytest

import helpers as Hh
import test_gpu_parity as TP
import test_gpu_quantised_disc as TQ
from ltgan import _cabi as K

BITS = {"step": 0, "one-call": 0, "step-generic": 1 << 18, "step-wide-grad": 1 << 14}
PREC = {"bf16": K.LTG_PREC_BF16, "fp32": K.LTG_PREC_FP32, "fp8": K.LTG_PREC_FP8}
ARITH = {"fp32": K.LTG_DARITH_FP32, "bf16x6": K.LTG_DARITH_BF16X6, "bf16x4": K.LTG_DARITH_BF16X4}
CONFIG_D = (100, 150, 250, 300)


def _cfg(I=500, hs=CONFIG_D, precision="bf16", tuning=0, d_precision="fp32", d_arith="bf16x6", item_lo=0, n_items_global=0):
    """item_lo / n_items_global: an item slab's two fields as Engine(item_lo, item_hi) fills them (0, 0: not sharded; I is then the LOCAL count)"""
    return K.ltg_config(I, 600, 200, n_items_global or I, *hs, PREC[precision], tuning, item_lo, n_items_global, PREC[d_precision], ARITH[d_arith],
                        1e-4, 0.9, 0.999, 1e-8, 1)


def g_route(precision, I, B, tuning=0, item_lo=0, n_items_global=0):
    """H = 600, Z = 200, a shadow of W_p1t, the lazy clock's pointers from 8 192 items on (as Engine hands them over); never dereferenced"""
    clock = I >= 8192
    gen = K.ltg_gen_state(wp1t_bf16=0x1000, q0_last=0x2000 if clock else None, q0_lr_hist=0x3000 if clock else None, q0_ord=0, q0_period=32 if clock else 0)
    out = K.ltg_g_route_info()
    cfg = _cfg(I, precision=precision, tuning=tuning, item_lo=item_lo, n_items_global=n_items_global)
    assert K.load().ltg_g_route(C.byref(cfg), C.byref(gen), B, C.byref(out)) == 1
    return out


def d_route(hs, n, with_bwd=True, d_precision="fp32", d_arith="bf16x6", tuning=0, has_aux=False, shadows=None, flat=True):
    """shadows: the fp8 operand-format copies; None = as Engine allocates them (fp8 and every layer size a multiple of 64).  flat: the eight
    tensors and their moments back to back from a 16-byte boundary (Engine's layout), else 8 bytes apart from it."""
    h0, h1, h2, h3 = hs
    sizes = [h0 * h1, h1, h0 * h2, h2, (h1 + h2) * h3, h3, h3, 1]

    def tensors(base):
        offs = [sum(sizes[:i]) * 4 + (0 if flat else 8 * i) for i in range(8)]
        return (K.vp * 8)(*[base + o for o in offs])
    if shadows is None:
        shadows = d_precision == "fp8" and all(x % 64 == 0 for x in hs)
    sh = [0x100000 * (k + 1) for k in range(5)] if shadows else [None] * 5
    disc = K.ltg_disc_state(0x10, tensors(0x10000000), tensors(0x20000000), tensors(0x30000000), *sh)
    out = K.ltg_d_route_info()
    cfg = _cfg(hs=hs, d_precision=d_precision, d_arith=d_arith, tuning=tuning)
    assert K.load().ltg_d_route(C.byref(cfg), C.byref(disc), n, int(with_bwd), int(has_aux), C.byref(out)) == 1
    return out


def _holds(route, want, tag):
    for k, v in want.items():
        got = getattr(route, k)
        got = list(got) if isinstance(v, list) else got
        assert got == v, (tag, k, got, v)


# ---- generator: the route classes the tables' comments name, field by field
def _tiles(dec_tile, dh2_tile, dw_tile):
    return dict(dec_tile=dec_tile, dh2=K.LTG_DH2_PARTIAL, dh2_tile=dh2_tile, dw=K.LTG_DW_TILE, dw_tile=dw_tile, dlog_bf16=0, sharded_ok=0)


FAST = dict(enc0=K.LTG_ENC0_FAST, small=0, mid=K.LTG_MID_FAST, loss=K.LTG_LOSS_COMBINE, grad_rows=1)
SMALL = dict(enc0=K.LTG_ENC0_FAST, small=1, mid=K.LTG_MID_FAST, dec=K.LTG_DEC_SMALL, loss=K.LTG_LOSS_ROW, dlog_bf16=0, dh2=K.LTG_DH2_SMALL,
             dw=K.LTG_DW_TAIL_JOB, q0=K.LTG_Q0_DENSE, q0_own_launch=0, sharded_ok=0)
SWEEP_IN_TAIL = dict(q0=K.LTG_Q0_SWEEP, q0_own_launch=0)
SWEEP_OWN = dict(q0=K.LTG_Q0_SWEEP, q0_own_launch=1)
LAZY = dict(q0=K.LTG_Q0_LAZY, q0_own_launch=1)


def MID(bf):
    """middle-layer fast path without streaming (4 096 < I < 8 192): 32 x 32 tiles, 16-byte loads when bf16 and I % 4 == 0; slot-map sweep in the tail"""
    t = -32 if bf else 32
    return dict(FAST, dec=K.LTG_DEC_TILE, stats=K.LTG_STATS_ROW, **_tiles(32, t, t), **SWEEP_IN_TAIL)


# large slab without the streaming kernels (fp32, or more than 128 rows): 64 x 128 / 64 x 64 tiles, fp32 dlog, segment pass, lazy clock
BIG_TILES = dict(FAST, dec=K.LTG_DEC_TILE, stats=K.LTG_STATS_SEGMENT, **_tiles(128, 128, 64), **LAZY)


def STREAM(form, ragged):
    return dict(FAST, dec=form, stats=K.LTG_STATS_EPILOGUE, dlog_bf16=1, dh2=K.LTG_DH2_STREAM, dw=K.LTG_DW_STREAM, dw_ragged=ragged, sharded_ok=1, **LAZY)


def GENERIC(bf, vec4=True):
    """tuning bit 18 below 8 192 items: generic everywhere"""
    t = -32 if (bf and vec4) else 32
    return dict(enc0=K.LTG_ENC0_GENERIC, small=0, mid=K.LTG_MID_DENSE, mid_vec=1, dec=K.LTG_DEC_TILE, stats=K.LTG_STATS_ROW, loss=K.LTG_LOSS_GENERIC,
                **_tiles(32, t, t), **SWEEP_OWN)


S1, S2 = K.LTG_DEC_STREAM1, K.LTG_DEC_STREAM2
G_ROUTES = {}
for p in ("fp32", "bf16"):
    bf = p == "bf16"
    for I, B in ((1000, 100), (1000, 256), (4096, 37), (4096, 100)):
        G_ROUTES[(p, I, B, 0)] = SMALL                                                          # small slab, up to 256 rows and 4 096 items
    # 257 rows: neither small nor middle-fast -- fk_enc0_fwd, k_dense_fwd, k_dec1_fwd, k_dlogits_combine, the five-launch backward
    for I in (1000, 4096):
        G_ROUTES[(p, I, 257, 0)] = dict(MID(bf), mid=K.LTG_MID_DENSE, **SWEEP_OWN)
    # I % 4 != 0: fk_dec1 but not the small-slab step; scalar loaders
    G_ROUTES[(p, 333, 17, 0)] = dict(MID(False), dec=K.LTG_DEC_SMALL, dec_tile=0)
    G_ROUTES[(p, 6000, 100, 0)] = G_ROUTES[(p, 6000, 64, 0)] = MID(bf)
    G_ROUTES[(p, 1000, 100, 1 << 18)] = GENERIC(bf)
    G_ROUTES[(p, 333, 17, 1 << 18)] = GENERIC(bf, vec4=False)
    for I, B in ((8200, 150), (8200, 300), (25024, 129)):                                       # more than 128 rows: not streaming
        G_ROUTES[(p, I, B, 0)] = dict(BIG_TILES, mid=K.LTG_MID_FAST if B <= 256 else K.LTG_MID_DENSE)
for I, B in ((8200, 100), (20000, 100), (25024, 100), (25024, 128), (25032, 100), (25032, 128), (200000, 100), (200008, 100)):
    G_ROUTES[("fp32", I, B, 0)] = BIG_TILES                                                     # fp32: not streaming
    G_ROUTES[("bf16", I, B, 0)] = STREAM(S2 if I >= 65536 else S1, int(I % 32 != 0))
G_ROUTES[("bf16", 65544, 16, 0)] = STREAM(S2, 1)                                                # the second form, chosen by the library
for I, B in ((8200, 100), (25032, 16)):
    G_ROUTES[("bf16", I, B, 1 << 17)] = STREAM(S2, 1)                                           # ... forced from 8 192 items
G_ROUTES[("bf16", 65544, 16, 1 << 26)] = STREAM(S1, 1)                                          # the first form again
G_ROUTES[("bf16", 8200, 100, 1 << 21)] = dict(STREAM(S1, 1), stats=K.LTG_STATS_SEGMENT)         # statistics from a second pass
G_ROUTES[("bf16", 8200, 100, 1 << 22)] = dict(STREAM(S1, 1), dlog_bf16=0, sharded_ok=0)         # fp32 dlog
G_ROUTES[("bf16", 25024, 128, 1 << 14)] = dict(STREAM(S1, 0), grad_rows=0)                      # column-blocked sparse gradient
# tuning bit 18 on a streaming-sized slab: the generic chain around the streaming decoder kernels (those do not depend on the bit), fp32 dlog
G_ROUTES[("bf16", 8200, 100, 1 << 18)] = dict(enc0=K.LTG_ENC0_GENERIC, small=0, mid=K.LTG_MID_DENSE, dec=S1, stats=K.LTG_STATS_EPILOGUE, loss=K.LTG_LOSS_GENERIC,
                                               dlog_bf16=0, dh2=K.LTG_DH2_STREAM, dw=K.LTG_DW_STREAM, dw_ragged=1, sharded_ok=0, **LAZY)
G_ROUTES[("fp32", 8200, 100, 1 << 18)] = dict(BIG_TILES, enc0=K.LTG_ENC0_GENERIC, mid=K.LTG_MID_DENSE, loss=K.LTG_LOSS_GENERIC)


# ---- item slabs (helpers.SLAB_G): the route of a rank is that of its LOCAL item count -- except that a slab is never "small": ltg_config.item_lo
# != 0 or n_items_global != n_items clears `small`, and with it loss (ROW -> COMBINE), dh2 (SMALL -> PARTIAL, 32-tiles), dw (TAIL_JOB -> TILE)
# and q0 (DENSE -> the slot-map sweep in the tail) move; dec stays the small decoder kernel (fk_dec1) up to 4 096 items.  Nothing else
# reads the two fields.  Keyed (precision, slab items): written out from the selection rules, like everything above.
def SLAB_SMALL_DEC(bf):
    """a slab of at most 4 096 items: the middle-fast chain around fk_dec1"""
    return dict(MID(bf), dec=K.LTG_DEC_SMALL, dec_tile=0)


SLAB_ROUTES = {}
for p in ("fp32", "bf16"):
    for n in (512, 488, 4040, 128):
        SLAB_ROUTES[(p, n)] = SLAB_SMALL_DEC(p == "bf16")
    SLAB_ROUTES[(p, 77)] = SLAB_SMALL_DEC(False)                                                 # 77 % 4 != 0: scalar loaders, 32-tiles
    SLAB_ROUTES[(p, 4160)] = MID(p == "bf16")                                                   # past RD_MAXI: the tiled decoder
for n in (8320, 8384):
    SLAB_ROUTES[("bf16", n)] = STREAM(S1, 0)
for n in (8200, 8264):
    SLAB_ROUTES[("bf16", n)] = STREAM(S1, 1)                                                    # n % 32 = 8: ragged tail of the weight update
# Slabs of ONE case that take different routes.  The replicated middle layers run the same kernels on every rank in all of them (mid, loss
# and the dz -> dh1 -> tail chain depend on the rows alone once no slab is "small"); what differs is slab-local:
#   8 200 / 2: 4 160 -> k_dec1_fwd 32-tiles, 4 040 -> fk_dec1             1 101 / 9 (fp32): one route; the kernels pick scalar loaders at 77 items
#   16 520 / 2: 8 320 -> no ragged tail, 8 200 -> ragged                  25 032 / 3: 8 384 x 2 -> none, 8 264 -> ragged
SLAB_SPLIT_ROUTES = {(8200, 2): ("dec", "dec_tile"), (1101, 9): (), (16520, 2): ("dw_ragged",), (25032, 3): ("dw_ragged",), (1000, 2): ()}


def _slab_cases():
    """(precision, slab items, B, item_lo, I) of every rank of every SLAB_G case"""
    return sorted({(p, hi - lo, B, lo, I) for p, I, B, R, _, _ in Hh.SLAB_G for lo, hi in Hh.slab_cuts(I, R)})


def test_every_slab_of_the_item_slab_cases_has_its_route_written_down():
    assert sorted({n for _, n, _, _, _ in _slab_cases()}) == [77, 128, 488, 512, 4040, 4160, 8200, 8264, 8320, 8384]
    for p, n, B, lo, I in _slab_cases():
        assert (p, n) in SLAB_ROUTES, (p, n)
        r = g_route(p, n, B, item_lo=lo, n_items_global=I)
        _holds(r, dict(SLAB_ROUTES[(p, n)], small=0), (p, n, B, lo, I))
        assert r.sharded_ok == int(n >= 8192)                    # the one-call step's cases: every slab of 16 520 / 2 and 25 032 / 3
    # the fields that differ between the slabs of one case are the ones named above, and none of them is read by a replicated layer
    fields = [f for f, _ in K.ltg_g_route_info._fields_]
    for (I, R), moving in SLAB_SPLIT_ROUTES.items():
        for p, B in {(p, B) for p, i, B, r, _, _ in Hh.SLAB_G if (i, r) == (I, R)}:
            routes = [g_route(p, hi - lo, B, item_lo=lo, n_items_global=I) for lo, hi in Hh.slab_cuts(I, R)]
            differ = {f for f in fields for x in routes[1:] if _field(x, f) != _field(routes[0], f)}
            assert differ - {"dh2_chunk", "dh2_nsplit"} == set(moving), (I, R, p, differ)
            assert not differ & {"enc0", "small", "mid", "mid_vec", "loss", "q0", "q0_own_launch", "grad_rows"}


def test_a_slab_is_never_small():
    """the same 512 items unsharded and as either slab of 1 000: item_lo / n_items_global move small, loss, dh2, dw, q0 -- and nothing else"""
    whole = g_route("bf16", 512, 100)
    _holds(whole, SMALL, "512 unsharded")
    for lo, Ig in ((0, 1000), (488, 1000)):
        r = g_route("bf16", 512, 100, item_lo=lo, n_items_global=Ig)
        moved = {f for f, _ in K.ltg_g_route_info._fields_ if _field(r, f) != _field(whole, f)}
        assert moved == {"small", "loss", "dh2", "dh2_tile", "dh2_chunk", "dh2_nsplit", "dw", "dw_tile", "q0"}, moved
    assert g_route("bf16", 512, 100, item_lo=0, n_items_global=512).small == 1      # the whole range named as a slab is not sharded


def _field(r, f):
    v = getattr(r, f)
    return v if isinstance(v, (int, float)) else list(v)


def _g_table_cases():
    """(precision, I, B, tuning) of every generator case of the GPU tables"""
    cases = [(p, I, B, knob) for I, B, p, knob, _ in Hh.HOT_FWD]
    cases += [(p, I, B, BITS[path]) for p, I, B, path, _ in Hh.HOT_G]
    cases += [(p, I, B, BITS[path]) for I, B, path, _ in TP.G_CASES for p in ("fp32", "bf16")]
    cases += [(p, I, B, BITS[path]) for p, I, B, path, _ in TP.G_SKEWED + TP.WARM_CASES]
    return sorted(set(cases))


@pytest.mark.parametrize("case", sorted(G_ROUTES), ids=lambda c: "%s-%d-%d-%#x" % c)
def test_generator_route(case):
    _holds(g_route(*case), G_ROUTES[case], case)


def test_every_generator_case_of_the_gpu_tables_has_its_route_written_down():
    missing = [c for c in _g_table_cases() if c not in G_ROUTES]
    assert not missing, missing
    # the one-call step: the tables run it where the library serves it (bf16), and check the refusal where it does not (fp32)
    for p, I, B, path in [(p, I, B, path) for p, I, B, path, _ in Hh.HOT_G + TP.G_SKEWED + TP.WARM_CASES] + \
                         [(p, I, B, path) for I, B, path, _ in TP.G_CASES for p in ("fp32", "bf16")]:
        if path == "one-call":
            assert g_route(p, I, B).sharded_ok == int(p == "bf16"), (p, I, B)


def test_generator_route_details():
    r = g_route("bf16", 8200, 100)
    assert (r.dh2_chunk, r.dh2_nsplit) == (256, 33)                  # 2 halves x 4 tiles of 32 items; 8 200 items in 33 slabs
    r = g_route("bf16", 6000, 100)
    assert (r.dh2_chunk, r.dh2_nsplit) == (256, 24)                  # ceil(6 000 / 64) = 94 -> 96 -> at least 256
    r = g_route("bf16", 200000, 100)
    assert (r.dh2_chunk, r.dh2_nsplit) == (2 * 800, 125)             # ceil(200 000 / 256) = 782 -> 800 items per half
    lib = K.load()
    for p, B, ok in (("bf16", 128, 1), ("fp32", 128, 0), ("bf16", 129, 0)):
        assert g_route(p, 25024, B).sharded_ok == ok
        gen = K.ltg_gen_state(wp1t_bf16=0x1000, q0_last=0x2000, q0_lr_hist=0x3000, q0_ord=0, q0_period=32)
        assert lib.ltg_g_step_sharded_ok(C.byref(_cfg(25024, precision=p)), C.byref(gen), B) == ok
    # without the clock's pointers: slot-map sweep as a launch of its own; without the shadow: no streaming
    cfg, out = _cfg(25024), K.ltg_g_route_info()
    assert lib.ltg_g_route(C.byref(cfg), C.byref(K.ltg_gen_state(wp1t_bf16=0x1000)), 100, C.byref(out)) == 1
    assert (out.q0, out.q0_own_launch, out.sharded_ok, out.dec) == (K.LTG_Q0_SWEEP, 1, 0, S1)
    assert lib.ltg_g_route(C.byref(cfg), C.byref(K.ltg_gen_state(q0_last=0x2000, q0_lr_hist=0x3000, q0_period=32)), 100, C.byref(out)) == 1
    assert (out.q0, out.dec, out.dec_tile, out.dlog_bf16) == (K.LTG_Q0_LAZY, K.LTG_DEC_TILE, 128, 0)


# ---- discriminator
# D_SIZES: kind of the step, and the tile codes (l1, l2, bwd1, bwd2) its comment states, at 40 pair rows; `promoted`: bwd1 takes 64 x 64
# tiles at 1 350 rows (more than 1 024 tiles of 32 x 32)
D_SIZE_ROUTES = {(99, 150, 250, 300): (K.LTG_D_GENERIC, [32, -32, -32, 32], True),
                 (100, 151, 250, 300): (K.LTG_D_GENERIC, [-33, 32, 32, -33], False),
                 (100, 150, 250, 301): (K.LTG_D_GENERIC, [-33, 32, 32, -33], False),
                 (100, 150, 250, 516): (K.LTG_D_GENERIC, [-33, -32, -32, -33], True),
                 (100, 150, 250, 324): (K.LTG_D_FAST, None, None),
                 (132, 150, 250, 300): (K.LTG_D_FAST, None, None),
                 (508, 256, 256, 128): (K.LTG_D_FAST, None, None),
                 (512, 256, 256, 128): (K.LTG_D_GENERIC, [64, -32, 64, 128], False),
                 (520, 300, 260, 132): (K.LTG_D_GENERIC, [64, -32, 64, 128], False),
                 (514, 300, 250, 130): (K.LTG_D_GENERIC, [32, 32, 32, 32], False),
                 (4, 1, 3, 4): (K.LTG_D_FAST, None, None),
                 (1, 1, 1, 1): (K.LTG_D_GENERIC, [32, 32, 32, 32], False)}


@pytest.mark.parametrize("hs,witness", TP.D_SIZES, ids=[TP._d_case_id(hs) for hs, _ in TP.D_SIZES])
def test_discriminator_route_of_every_layer_size(hs, witness):
    kind, tiles, promoted = D_SIZE_ROUTES[hs]
    assert witness is None or (witness == "fast") == (kind == K.LTG_D_FAST)      # the table's own witness says the same
    for n in (40, 1350):
        for arith in ("fp32", "bf16x6"):
            r = d_route(hs, n, d_arith=arith)
            assert r.kind == kind and r.mode == 0, (hs, n, arith, r.kind)
            if tiles is not None:
                want = list(tiles)
                if promoted and n == 1350:
                    want[2] = 64
                assert list(r.tile) == want, (hs, n, list(r.tile), want)
            if kind == K.LTG_D_FAST:                                              # the library's split set: l2, bwd1, bwd2
                assert list(r.spl) == ([0, 0, 0, 0] if arith == "fp32" else [0, 6, 6, 6]) and r.adam == K.LTG_D_ADAM_FLAT
        assert d_route(hs, n, tuning=1 << 18).kind == K.LTG_D_GENERIC
        assert d_route(hs, n, d_precision="bf16").kind == K.LTG_D_GENERIC and d_route(hs, n, d_precision="bf16").mode == 1


def test_discriminator_step_cases_of_the_gpu_tables():
    for nr, nf, hs in TP.D_STEP_CASES:
        if hs is None:       # _d_step_case's own choice
            hs = (2048, 1024, 512, 256) if nr == 260 else (CONFIG_D if nr > 300 else (12, 20, 28, 16))
        want = D_SIZE_ROUTES[hs][0] if hs in D_SIZE_ROUTES else (K.LTG_D_GENERIC if hs[0] == 2048 else K.LTG_D_FAST)
        assert d_route(hs, nr + nf).kind == want, (nr, nf, hs)
    r = d_route((2048, 1024, 512, 256), 510)                                      # BASELINE config 5, fp32: the wide tiles, per-tensor Adam
    assert list(r.tile) == [64, -32, 64, 128] and r.adam == K.LTG_D_ADAM_TENSORS
    assert list(d_route(CONFIG_D, 1850, d_arith="bf16x4").spl) == [4, 4, 4, 4]


def test_forward_only_tower_routes():
    for hs in (CONFIG_D, (4, 1, 3, 4)):
        assert d_route(hs, 100, with_bwd=False, d_arith="bf16x6").kind == K.LTG_D_TOWER
        assert d_route(hs, 100, with_bwd=False, d_arith="bf16x4").kind == K.LTG_D_TOWER
    assert d_route(CONFIG_D, 100, with_bwd=False, d_arith="fp32").kind == K.LTG_D_STAGED_FWD
    assert d_route(CONFIG_D, 100, with_bwd=False, tuning=1 << 20).kind == K.LTG_D_STAGED_FWD
    for hs in ((100, 150, 250, 324), (132, 150, 250, 300)):                       # past the tower's h3 / h0 limits
        assert d_route(hs, 100, with_bwd=False).kind == K.LTG_D_STAGED_FWD
    assert d_route((4, 1, 3, 4), 100, with_bwd=False, d_arith="fp32").kind == K.LTG_D_FAST        # h0 < 32: fk_d_l1 -> fk_d_l2 -> fk_d_y
    assert d_route((1, 1, 1, 1), 100, with_bwd=False).kind == K.LTG_D_GENERIC
    assert d_route((512, 256, 256, 128), 100, with_bwd=False).kind == K.LTG_D_GENERIC
    assert d_route(CONFIG_D, 100, with_bwd=False, tuning=1 << 18).kind == K.LTG_D_GENERIC


# fp8: (layer sizes) -> kind of the step as Engine runs it
Q_ROUTES = {TQ.OPFMT: K.LTG_D_FP8_OPFMT, TQ.BASE: K.LTG_D_FP8_OPFMT,
            (512, 256, 256, 640): K.LTG_D_FP8_STAGED,      # h3 beyond the operand-format output kernel
            (192, 64, 128, 128): K.LTG_D_FP8_REG,          # multiples of 64 but not of 128
            (256, 128, 128, 100): K.LTG_D_GENERIC,         # h3 no multiple of 64: Engine builds no shadows
            (520, 300, 260, 132): K.LTG_D_GENERIC, (514, 300, 250, 130): K.LTG_D_GENERIC, (100, 151, 250, 300): K.LTG_D_GENERIC,
            (4, 1, 3, 4): K.LTG_D_GENERIC, (1, 1, 1, 1): K.LTG_D_GENERIC}


def test_quantised_discriminator_routes():
    for dq, hs, nr, nf in TQ.D_Q:
        r = d_route(hs, nr + nf, d_precision=dq)
        if dq == "bf16":
            assert (r.kind, r.mode) == (K.LTG_D_GENERIC, 1), (hs, nr, nf)
        else:
            assert (r.kind, r.mode) == (Q_ROUTES[hs], 2), (hs, nr, nf, r.kind)
            assert r.adam == (K.LTG_D_ADAM_FP8 if r.kind == K.LTG_D_FP8_OPFMT else K.LTG_D_ADAM_TENSORS)
    assert d_route((100, 150, 250, 300), 1850, d_precision="bf16").tile[2] == 64                 # D_Q's last case: bwd1 promoted, t32 = 1 794
    assert d_route(TQ.OPFMT, 1025, d_precision="fp8", tuning=1 << 19).kind == K.LTG_D_FP8_STAGED # backward converts on the fly
    assert d_route(TQ.OPFMT, 1025, d_precision="fp8", with_bwd=False).kind == K.LTG_D_FP8_STAGED # forward only: no operand-format step
    # a caller that hands shadows over at h3 = 100 (the forward layers contract over h0 and h1 + h2 only): staged forward + generic backward
    assert d_route((256, 128, 128, 100), 40, d_precision="fp8", shadows=True).kind == K.LTG_D_FP8_STAGED
    assert list(d_route((512, 256, 256, 640), 40, d_precision="fp8").tile) == [64, 64, 64, 128]  # fp8: l2 on 64-tiles as well


def test_fork_of_jobs_b_and_c():
    """from 1 024 pair rows, with an aux stream and device words, and only with the flat tensor layout"""
    assert d_route(CONFIG_D, 1024, has_aux=True).fork == 1
    assert d_route(CONFIG_D, 1023, has_aux=True).fork == 0
    assert d_route(CONFIG_D, 1024, has_aux=False).fork == 0
    r = d_route(CONFIG_D, 1024, has_aux=True, flat=False)
    assert (r.fork, r.adam) == (0, K.LTG_D_ADAM_TENSORS)
    assert d_route(CONFIG_D, 1024, has_aux=True, with_bwd=False).fork == 0
    assert d_route((512, 256, 256, 128), 2048, has_aux=True).fork == 0            # not the fk_d_* step
