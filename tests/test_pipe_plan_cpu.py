"""The schedule of the one-call G step for every pipe mode (include/ltg.h: ltg_g_pipe_plan; host-only, no GPU).

ltg_g_step_sharded decides once per call where each stage runs and what it waits for (csrc/ltg_kernels.hip: pipe_plan), and its stages, the
host's bookkeeping (Engine.g_step_sharded, Engine._pipe_ready) and ltg_g_pipe_join read that one struct.  This module pins the struct for
the modes the GPU tests drive through LTG_PIPE_* / LTGAN_*.  The expected values are written out from the rules as they stood inline in
ltg_g_step_sharded before the plan existed (eleven booleans derived from ltg_pipe.flags and pointer presence), not computed by a second
copy of them.  The pointers below are distinct fake addresses and are never dereferenced."""
import ctypes as C
import os
import re

import pytest

from ltgan import _cabi as K

W, E, O = K.LTG_HAND_WORDS, K.LTG_HAND_EVENTS, K.LTG_HAND_ORDER
SIDE, TOUCH, OWN = K.LTG_SLICE_SIDE, K.LTG_SLICE_IN_TOUCH, K.LTG_SLICE_OWN_END
FIELDS = ("handover", "slice", "ahead", "shadow", "h2_early", "tail_own", "grad_rows", "poisonable")


def fake(k):
    return 0x10000 * (k + 1)


def _arr(o):
    return (K.vp * 8)(*[fake(o + i) for i in range(8)])


def cfg(I=25024):
    """the configuration of test_cabi's plan test: H 600, Z 200, bf16"""
    return K.ltg_config(I, 600, 200, I, 100, 150, 250, 300, K.LTG_PREC_BF16, 0, 0, 0, K.LTG_PREC_FP32, 0, 1e-4, 0.9, 0.999, 1e-8, 1)


GEN = K.ltg_gen_state(_arr(0), _arr(8), _arr(16), fake(30), fake(31), fake(32), 0, 32)     # a shadow of W_p1t, a clock with period 32


def batch(rows=100, uitem=fake(46)):
    return K.ltg_batch(rows, 50, fake(40), fake(41), None, None, fake(42), fake(43), fake(44), fake(45), uitem)


def pipe(flags=0, sync=fake(50), mark=fake(51), shadow=fake(52), tail=None, ev_tail=None):
    return K.ltg_pipe(fake(60), fake(61), fake(62), ev_tail, fake(63), fake(64), fake(65), flags, 1, sync, tail, mark, None, 0, 0, shadow)


def plan(p, b=None, c=None):
    """the filled struct, or None when the call would be refused; ltg_g_step_sharded_plan's bits are its projection either way"""
    lib, b, c = K.load(), b or batch(), c or cfg()
    out = K.ltg_pipe_plan_info()
    ok = lib.ltg_g_pipe_plan(C.byref(c), C.byref(GEN), C.byref(b), C.byref(p), C.byref(out))
    bits = lib.ltg_g_step_sharded_plan(C.byref(c), C.byref(GEN), C.byref(b), C.byref(p))
    assert ok in (0, 1)
    assert bits == ((K.LTG_PLAN_AHEAD if out.ahead else 0) | (K.LTG_PLAN_SHADOW if out.shadow else 0) if ok else 0), (bits, ok)
    return out if ok else None


def _holds(got, want, tag):
    assert got is not None, tag
    for k, v in zip(FIELDS, want):
        if v is not None:
            assert getattr(got, k) == v, (tag, k, getattr(got, k), v)


# (None: the case pins no value for the field)          handover slice  ahead shadow h2_early tail_own grad_rows poisonable
MODES = [
    ("flags 0", dict(),                                      (W, SIDE, 1, 1, 1, 0, 1, 1)),
    ("EVENTS", dict(flags=K.LTG_PIPE_EVENTS),                (E, TOUCH, 0, 0, 0, 0, 1, 0)),
    ("sync == NULL", dict(sync=None),                        (E, TOUCH, 0, 0, 0, 0, 1, 0)),
    ("NO_DEC1_FORK", dict(flags=K.LTG_PIPE_NO_DEC1_FORK),    (O, OWN, 0, 0, 0, 0, None, 0)),
    ("NO_SLICE_FORK", dict(flags=K.LTG_PIPE_NO_SLICE_FORK),  (W, OWN, 0, 1, None, 0, None, None)),
    ("SLICE_IN_TOUCH", dict(flags=K.LTG_PIPE_SLICE_IN_TOUCH), (W, TOUCH, 0, 1, None, 0, None, None)),
]


@pytest.mark.parametrize("tag,kw,want", MODES, ids=[m[0] for m in MODES])
def test_every_pipe_mode_has_its_schedule_written_down(tag, kw, want):
    _holds(plan(pipe(**kw)), want, tag)


def test_the_struct_is_eight_int32_fields_in_the_headers_order():
    assert C.sizeof(K.ltg_pipe_plan_info) == 32
    assert [f[0] for f in K.ltg_pipe_plan_info._fields_] == ["handover", "slice", "ahead", "shadow", "tail_own", "h2_early", "grad_rows", "poisonable"]
    assert (O, E, W) == (0, 1, 2) and (OWN, TOUCH, SIDE) == (0, 1, 2)


def test_wide_grad_switches_the_sparse_gradient_to_its_column_blocked_shape():
    assert plan(pipe(flags=K.LTG_PIPE_WIDE_GRAD)).grad_rows == 0
    assert plan(pipe()).grad_rows == 1


def _csrc_constant(name):
    src = ""
    for fn in ("ltg_gstep.h", "ltg_fast_gen.h"):
        src += open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "long-tail-gan_amd", "csrc", fn)).read()
    m = re.search(r"\b%s = (\d+)" % name, src)
    assert m, name
    return int(m.group(1))


def test_the_tail_runs_on_its_own_stream_only_when_asked_given_and_able():
    """LTG_PIPE_TAIL_OWN needs the tail stream and its event, the row-wave gradient kernel (not WIDE_GRAD) and at most G0_LIGHT batch rows per
    partial bias row (ENC0_BIAS_PARTS of them): 16 x 8 = 128 rows.  That is also the most rows the one-call step serves at all, so
    "just above the bound" is a call the library refuses: no plan, and in particular no tail of its own."""
    parts, light = _csrc_constant("ENC0_BIAS_PARTS"), _csrc_constant("G0_LIGHT")
    assert (parts, light) == (8, 16)
    own = dict(flags=K.LTG_PIPE_TAIL_OWN, tail=fake(70), ev_tail=fake(71))
    for rows in (100, parts * light - 1, parts * light):
        _holds(plan(pipe(**own), batch(rows)), (W, SIDE, 1, 1, 1, 1, 1, 1), rows)
    lib, out = K.load(), K.ltg_pipe_plan_info()
    above = batch(parts * light + 1)
    assert lib.ltg_g_pipe_plan(C.byref(cfg()), C.byref(GEN), C.byref(above), C.byref(pipe(**own)), C.byref(out)) == 0 and out.tail_own == 0
    assert plan(pipe(**own), above) is None
    assert plan(pipe(flags=K.LTG_PIPE_TAIL_OWN)).tail_own == 0                                  # no tail stream
    assert plan(pipe(flags=K.LTG_PIPE_TAIL_OWN, tail=fake(70))).tail_own == 0                   # ... or no event to join it with
    assert plan(pipe(tail=fake(70), ev_tail=fake(71))).tail_own == 0                            # not asked for
    wide = plan(pipe(flags=K.LTG_PIPE_TAIL_OWN | K.LTG_PIPE_WIDE_GRAD, tail=fake(70), ev_tail=fake(71)))
    assert wide.tail_own == 0 and wide.grad_rows == 0
    for fl in (K.LTG_PIPE_EVENTS, K.LTG_PIPE_SLICE_IN_TOUCH, K.LTG_PIPE_NO_SLICE_FORK, K.LTG_PIPE_NO_DEC1_FORK):   # only beside the slice on the side stream
        assert plan(pipe(flags=K.LTG_PIPE_TAIL_OWN | fl, tail=fake(70), ev_tail=fake(71))).tail_own == 0, fl


def test_the_catch_up_ahead_needs_marks_and_the_batchs_item_list():
    assert plan(pipe(), batch(uitem=None)).ahead == 0
    assert plan(pipe(mark=None)).ahead == 0
    _holds(plan(pipe(mark=None)), (W, SIDE, 0, 1, 1, 0, 1, 1), "no q0_mark")                    # nothing else moves


def test_the_second_shadow_buffer_must_be_a_second_buffer():
    assert plan(pipe(shadow=fake(30))).shadow == 0                                              # shadow_out == gen.wp1t_bf16: in place
    assert plan(pipe(shadow=None)).shadow == 0
    _holds(plan(pipe(shadow=fake(30))), (W, SIDE, 1, 0, 1, 0, 1, 1), "in place")


def test_a_ragged_slab_opens_the_h2_word_with_the_updates_end():
    """9 000 items (the slab of the lazy-clock GPU test): the last 9 000 % 32 rows go through the generic tile kernel, which reads h2 throughout"""
    _holds(plan(pipe(), c=cfg(9000)), (W, SIDE, 1, 1, 0, 0, 1, 1), "9 000 items")
    assert plan(pipe(), c=cfg(9024)).h2_early == 1


def test_calls_the_step_refuses_have_no_plan():
    for bit in (64, 1 << 8, 4):                                                                 # outside LTG_PIPE_*
        assert plan(pipe(flags=bit)) is None, bit
    assert plan(pipe(), c=cfg(1000)) is None                                                    # a small slab: ltg_g_step_sharded_ok refuses it
    assert plan(pipe(flags=K.LTG_PIPE_TAIL_OWN | K.LTG_PIPE_WIDE_GRAD | K.LTG_PIPE_SLICE_IN_TOUCH | K.LTG_PIPE_EVENTS | K.LTG_PIPE_NO_SLICE_FORK | K.LTG_PIPE_NO_DEC1_FORK)) is not None


def test_a_library_without_the_plan_query_gets_the_same_bookkeeping_from_the_host():
    """Engine.pipe_plan over a build that has only ltg_g_step_sharded_plan (an older library loaded for A/B timing): the four fields the host
    reads -- handover, ahead, shadow, tail_own (there: asked for and given a stream) -- as the library's own plan has them, for every mode."""
    import types
    from ltgan.engine import Engine
    lib = K.load()
    old = types.SimpleNamespace(ltg_g_step_sharded_plan=lib.ltg_g_step_sharded_plan)
    own = dict(tail=fake(70), ev_tail=fake(71))
    for kw in [m[1] for m in MODES] + [dict(mark=None), dict(shadow=None), dict(flags=K.LTG_PIPE_TAIL_OWN, **own),
                                       dict(flags=K.LTG_PIPE_TAIL_OWN | K.LTG_PIPE_EVENTS, **own), dict(flags=K.LTG_PIPE_TAIL_OWN)]:
        p = pipe(**kw)
        want = plan(p)
        got = Engine.pipe_plan(types.SimpleNamespace(lib=old, cfg=cfg(), gen_c=GEN), types.SimpleNamespace(c=batch()), types.SimpleNamespace(c=p))
        assert [(k, getattr(got, k)) for k in ("handover", "ahead", "shadow", "tail_own")] == \
               [(k, getattr(want, k)) for k in ("handover", "ahead", "shadow", "tail_own")], kw
    bare = Engine.pipe_plan(types.SimpleNamespace(lib=types.SimpleNamespace(), cfg=cfg(), gen_c=GEN), types.SimpleNamespace(c=batch()), types.SimpleNamespace(c=pipe()))
    assert (bare.handover, bare.ahead, bare.shadow) == (W, 0, 0)                                # before the plan bits existed: neither
