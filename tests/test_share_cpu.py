"""CPU-side checks of the share-targeted lists: ltg_share_ws_bytes / ltg_topk_share are exported and bound with the header's argument types,
every documented refusal returns LTG_EINVAL without a GPU, ShareTarget and the Recommender validate, both CLIs handle --share, the extra
summary line, and the numpy reference the GPU tests lean on (tests/share_ref.py): against a brute force over every allocation of steps
its total step cost is the least, and its tables have the consequences DESIGN 5.17 lists."""
import ctypes as C
import os

import numpy as np
import pytest

import share_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_entry_points_are_exported_and_bound_with_the_headers_types():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    want = {"ltg_share_ws_bytes": (sz, [i32, i32]),
            "ltg_topk_share": (C.c_int, [i32, i32, vp, vp, vp, vp, i32, i64, vp, vp, vp, vp, sz, vp])}
    for name, (res, args) in want.items():
        assert cabi.SYMBOLS[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res, name
    assert cabi.LTG_SHARE_STATE == 8
    assert lib.ltg_abi_version() == 14 == cabi.LTG_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ltg.h")).read()
    assert "#define LTG_SHARE_STATE 8" in header and "#define LTG_ABI_VERSION 14" in header
    assert "size_t ltg_share_ws_bytes(int32_t n_rows, int32_t k);" in header
    assert "int ltg_topk_share(int32_t n_rows, int32_t m_in, const float* score_pro, const int32_t* id_pro, const float* score_rest," in header
    assert "const int32_t* id_rest, int32_t k, int64_t want, float* score_out, int32_t* id_out," in header
    kernel = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_share.h")).read()
    assert "constexpr int SH_STATE = 8;" in kernel
    hip = open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "ltg_kernels.hip")).read()
    assert hip.index('#include "ltg_cap.h"') < hip.index('#include "ltg_share.h"')
    assert "ltg_share.h" in open(os.path.join(ROOT, "long-tail-gan_amd", "csrc", "Makefile")).read()


def test_ws_bytes_helper():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    assert lib.ltg_share_ws_bytes(10, 8) >= 80 * 8 + 2 * 10 * 4 + 8 * 256 * 4
    assert lib.ltg_share_ws_bytes(0, 1) > 0
    assert lib.ltg_share_ws_bytes(3000, 100) < lib.ltg_share_ws_bytes(3001, 100) < lib.ltg_share_ws_bytes(3001, 101)
    assert lib.ltg_share_ws_bytes(20000, 100) < lib.ltg_share_ws_bytes(20000, 1024)
    for bad in ((-1, 8), (10, 0), (10, -1), (10, 1025), (2 ** 21, 1024), (2 ** 30, 2), (2 ** 31 - 1, 2)):
        assert lib.ltg_share_ws_bytes(*bad) == 0, bad
    assert lib.ltg_share_ws_bytes(2 ** 21 - 1, 1024) > 0 and lib.ltg_share_ws_bytes(2 ** 31 - 1, 1) > 0


def test_refusals_without_gpu():
    from ltgan import _cabi as cabi
    lib = cabi.load()
    new_f, new_i = (lambda: (C.c_float * 64)()), (lambda: (C.c_int32 * 64)())
    ps, rs, so, pi, ri, io, st, ws = new_f(), new_f(), new_f(), new_i(), new_i(), new_i(), (C.c_int32 * 8)(), (C.c_uint8 * 8)()
    big = 1 << 40                                        # (never dereferenced: every call below is refused or has no rows)

    def share(n=2, m=8, ps=ps, pi=pi, rs=rs, ri=ri, k=4, want=3, so=so, io=io, state=st, w=ws, wb=big):
        return lib.ltg_topk_share(n, m, ps, pi, rs, ri, k, want, so, io, state, w, wb, None)

    st[:] = [-9] * 8
    assert share(n=0) == 0 and list(st) == [-9] * 8      # zero rows: nothing to launch, no state written
    for name in ("ps", "pi", "rs", "ri", "so", "io", "state", "w"):
        assert share(**{name: None}) == -1, name
        assert share(n=0, **{name: None}) == -1, name    # ... but the arguments are still checked
    for kw in (dict(n=-1), dict(n=2 ** 28, m=8, k=8), dict(n=2 ** 21, m=1024, k=1024), dict(wb=lib.ltg_share_ws_bytes(2, 4) - 1)):
        assert share(**kw) == -1, kw
    for kw in (dict(m=0), dict(m=-1), dict(m=1025, k=1025), dict(m=1025), dict(k=0), dict(k=-1), dict(k=9), dict(k=2 ** 31 - 1), dict(want=-1),
               dict(want=-2 ** 40), dict(wb=0), dict(wb=lib.ltg_share_ws_bytes(0, 4) - 1)):
        assert share(**kw) == -1 and share(n=0, **kw) == -1, kw
    for kw in (dict(m=1024, k=1024, wb=lib.ltg_share_ws_bytes(0, 1024)), dict(k=8), dict(k=1), dict(want=0), dict(want=2 ** 40)):
        assert share(n=0, **kw) == 0, kw
    # an output that is, or overlaps, an input
    for kw in (dict(so=ps), dict(so=rs), dict(io=pi), dict(io=ri), dict(so=pi), dict(io=rs)):
        assert share(**kw) == -1 and share(n=0, **kw) == -1, kw
    inside = C.cast(C.addressof(ps) + 16, C.c_void_p)    # four floats into the promoted scores
    assert share(so=inside) == -1
    assert list(st) == [-9] * 8


class _FakeEngine:
    I, I_global, device, item_lo = 50, 50, "cpu", 0

    def share_ws_bytes(self, n, k):
        return 64


def test_share_target_validation():
    from ltgan.serving import group_mask_of
    from ltgan.sharded import ShareTarget as ShardedShareTarget
    from ltgan.trainer import Calibrate, Diversify, ExposureCap, Recommender, ShareTarget
    assert ShardedShareTarget is ShareTarget
    labels = np.array([0, 1, 7] * 16 + [0, 0], np.uint8)
    for n_groups in (0, 9):
        with pytest.raises(ValueError):
            ShareTarget(labels, n_groups, [0], 0.3)
    for promote in ([], [2], [-1], [0, 5]):
        with pytest.raises(ValueError):
            ShareTarget(labels, 2, promote, 0.3)
    for share in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ShareTarget(labels, 2, [1], share)
    with pytest.raises(ValueError):
        ShareTarget(labels[:49], 2, [1], 0.3).bind(_FakeEngine(), 10, 10, 33)   # a label count that differs from the catalogue
    with pytest.raises(ValueError):
        ShareTarget(labels, 2, [1], 0.3).bind(_FakeEngine(), 10, 1024, 2 ** 21)  # 2^21 users x 1024 entries: 2^31 steps
    with pytest.raises(ValueError):
        ShareTarget(labels, 2, [1], 0.3).bind(_FakeEngine(), 10, 1025, 3)
    t = ShareTarget(labels, 2, [1], 0.3)
    t.bind(_FakeEngine(), 10, 10, 33)
    assert t.mask == group_mask_of([1], 2) == 0b10 and t.rest_mask == 0x1FF & ~0b10 and t.rest_mask & 0x100
    assert t.want == int(np.ceil(np.float64(0.3) * 33 * 10)) == 99
    assert tuple(t.pro_i.shape) == tuple(t.rest_s.shape) == (33, 10) and t.state.numel() == 8
    t = ShareTarget(labels, 3, [2, 0, 2], 1.0)
    t.bind(_FakeEngine(), 10, 7, 5)
    assert t.promote == [0, 2] and t.mask == 0b101 and t.rest_mask == 0x1FA and t.want == 35
    assert ShareTarget(labels, 2, [0], 0.0).share == 0.0
    good = ShareTarget(labels, 2, [1], 0.3)
    for kw in (dict(rule=object()), dict(diversify=Diversify(0.5)), dict(calibrate=Calibrate(labels, 2, 0.5)), dict(cap=ExposureCap(5))):
        with pytest.raises(ValueError):                  # refused before anything of the engine is touched
            Recommender(_FakeEngine(), None, k=10, share=good, **kw)
    with pytest.raises(ValueError):
        Recommender(_FakeEngine(), None, k=0, share=good)


def test_cli_arguments():
    from ltgan import longtail as lt
    from ltgan import recommend as rc
    for mod in (rc, lt):
        a = mod.parse_args(["ds", "model.pt"])                           # nothing changes without the option
        assert a.share is None and a.shares is None
        assert mod.parse_args(["ds", "m.pt", "--share", "niche:0.3"]).shares == ([1], 0.3)
        assert mod.parse_args(["ds", "m.pt", "--share", "popular:0"]).shares == ([0], 0.0)
        assert mod.parse_args(["ds", "m.pt", "--share", "niche+popular:1"]).shares == ([0, 1], 1.0)
        assert mod.parse_args(["ds", "m.pt", "--share", "pop3+pop1:0.25", "--groups", "pop:4"]).shares == ([1, 3], 0.25)
        for bad in (["--share"], ["--share", "niche"], ["--share", "0.3"], ["--share", ":0.3"], ["--share", "niche:"], ["--share", "niche:x"],
                    ["--share", "niche:-0.1"], ["--share", "niche:1.5"], ["--share", "niche:nan"], ["--share", "rare:0.3"],
                    ["--share", "niche+niche:0.3"], ["--share", "niche+:0.3"], ["--share", "pop0:0.3"], ["--share", "niche,popular:0.3"],
                    ["--share", "niche:0.3", "--min-slots", "niche:5"], ["--share", "niche:0.3", "--diversify", "0.5"],
                    ["--share", "niche:0.3", "--calibrate", "0.5"], ["--share", "niche:0.3", "--cap", "5"]):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(["ds", "m.pt"] + bad)
            assert e.value.code == 2, (mod.__name__, bad)
    assert rc.parse_args(["ds", "m.pt", "--share", "niche:0.5", "--explain", "3"]).explain == 3     # the explanations read the final lists
    assert lt.parse_share("b+a: 0.5", ["a", "b"]) == ([0, 1], 0.5)


def test_share_line_from_hand_made_stats():
    from ltgan import longtail as lt
    st = dict(plain_share=0.125, share=0.3, target=0.3, taken=70, available=900, rows_changed=12, price=0.75, reached=True)
    assert lt.share_line(["niche"], st, 100) == "share@100: niche 0.125000 -> 0.300000 (target 0.300000), 12 rows changed, price 0.75"
    assert lt.share_line(["pop2", "pop3"], dict(st, price=0.0), 20).startswith("share@20: pop2+pop3 0.125000 -> ")


# ---------------------------------------------------------------------------------------------- the reference
def tiny_cases():
    """3 users, 9 items, k = 4; every other case with scores quantised to 0.5, so that equal and +-0 costs occur"""
    for seed in range(200):
        yield seed, S.share_case(3, 9, 4, 9, quant=0.5 if seed % 2 else None, seed=500 + seed)[:4]


def test_the_reference_is_the_cheapest_allocation():
    zero_costs = negative_zero = 0
    for seed, (ps, pi, rs, ri) in tiny_cases():
        _, _, st0, ex0 = S.share_lists(ps, pi, rs, ri, 4, 0)
        A, N = int(st0[0]), int(st0[1])
        for u in range(3):                               # the raw differences: -0.0 does occur, and the word takes it as +0.0
            a, kk, w = S.row_steps(ps[u], pi[u], rs[u], ri[u], 4, u)
            b = kk - a
            for t in range(1, len(w) + 1):
                c = np.float32(rs[u][b - t]) - np.float32(ps[u][a + t - 1])
                assert c >= 0, (seed, u, t)
                negative_zero += int(c == 0 and np.signbit(c))
                zero_costs += int(c == 0)
                assert int(w[t - 1]) >> 32 == (0 if c == 0 else int(np.float32(c).view(np.uint32)))
            assert (np.diff(w.astype(object)) > 0).all() if len(w) > 1 else True        # a row's words strictly increase
        for want in range(A, A + N + 2):
            s, i, st, ex = S.share_lists(ps, pi, rs, ri, 4, want)
            take = min(want - A, N)
            assert st[2] == take == int(ex["t"].sum()), (seed, want)
            assert S.step_cost(ex["words"], ex["t"]) == S.cheapest_allocation(ex["words"], take), (seed, want)
            promoted = sum(int(np.isin(i[u][i[u] >= 0], pi[u][pi[u] >= 0]).sum()) for u in range(3))
            assert promoted == A + take == min(want, A + N), (seed, want)
    assert zero_costs > 0


def test_minus_zero_against_plus_zero_sorts_first():
    """rest = -0.0 against pro = +0.0: the difference is -0.0, whose bits would sort last; taken as +0.0 it is the cheapest step"""
    ps = np.array([[0.0], [1.0]], np.float32)
    pi = np.array([[1], [1]], np.int32)
    rs = np.array([[-0.0], [1.5]], np.float32)
    ri = np.array([[0], [0]], np.int32)
    assert np.signbit(np.float32(rs[0, 0] - ps[0, 0]))
    s, i, st, ex = S.share_lists(ps, pi, rs, ri, 1, 1)
    assert st.tolist() == [0, 2, 1, 1, 0, 2, 0, 0] and i[:, 0].tolist() == [1, 0] and ex["t"].tolist() == [1, 0]
    assert _bits(s[:, 0]).tolist() == _bits(np.array([0.0, 1.5], np.float32)).tolist()


def test_consequences_of_the_definition():
    for n, I, k, c, quant in ((64, 40, 5, 40, None), (130, 70, 33, 70, None), (211, 129, 10, 129, 0.5), (60, 300, 20, 35, None)):
        ps, pi, rs, ri, _ = S.share_case(n, I, k, c, quant=quant)
        p0s, p0i, st0, ex0 = S.share_lists(ps, pi, rs, ri, k, 0)
        A, N = int(st0[0]), int(st0[1])
        assert st0.tolist() == [A, N, 0, 0, 0, int(ex0["kk"].sum()), 0, 0] and N > 0
        for u in range(n):                               # the plain list is the merge of everything, cut to kk
            s, i, _ = S.merged(ps[u], pi[u], rs[u], ri[u], S.list_len(pi[u]), S.list_len(ri[u]))
            kk = int(ex0["kk"][u])
            assert np.array_equal(p0i[u, :kk], i[:kk]) and np.array_equal(_bits(p0s[u, :kk]), _bits(s[:kk]))
        s, i, st, _ = S.share_lists(ps, pi, rs, ri, k, A)                # a target the plain lists meet
        assert np.array_equal(i, p0i) and np.array_equal(_bits(s), _bits(p0s)) and st[2] == 0
        full = S.share_lists(ps, pi, rs, ri, k, A + N)
        beyond = S.share_lists(ps, pi, rs, ri, k, A + N + 1000)
        assert full[2][2] == N and np.array_equal(full[1], beyond[1]) and np.array_equal(full[2], beyond[2])
        assert all(len(w) == t for w, t in zip(full[3]["words"], full[3]["t"]))          # every row at its limit
        last = 0
        for want in np.linspace(A, A + N, 7).astype(int):
            s, i, st, ex = S.share_lists(ps, pi, rs, ri, k, int(want))
            promoted = 0
            for u in range(n):
                got = i[u][i[u] >= 0]
                assert len(set(got.tolist())) == len(got) == ex["kk"][u]
                w = S.order_words(s[u, :len(got)], got).astype(object)
                assert (np.diff(w) < 0).all() if len(w) > 1 else True                   # ltg_topk's order
                promoted += int(np.isin(got, pi[u][:S.list_len(pi[u])]).sum())
            assert promoted == want and st[2] == want - A
            price = int(st[4])
            assert price >= last                                                         # a larger target never lowers the price
            last = price
