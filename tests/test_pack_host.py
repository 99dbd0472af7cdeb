"""The packed-weight formats on the CPU: tests/pack_ref.py's sizes equal the library's host functions; unpack(pack(w)) == w
for every format and direction; the comparison rule of tests/test_gpu_pack.py rejects an fp32 evaluation of either Winograd
transform, unreversed backward taps, two exchanged slices, a chunk shifted by one and a non-zero padding element, and
accepts a double evaluation in another order; the tables of pack_all's three launches (ops._pack_rows) and, with the
launches stubbed out, the cache rules of ops/packing.py."""
import numpy as np
import pytest
import torch

import pack_ref as pr

# channel counts: every value up to 80, then the multiples of 8 with both neighbours (every tile / chunk edge) up to 700
GRID = sorted(set(range(1, 81)) | {m + d for m in range(80, 697, 8) for d in (-1, 0, 1)} | {700})
SHAPES = [(65, 9), (6, 64), (63, 7), (96, 40)]                      # (Cout, Cin): partial and whole tiles / chunks


@pytest.fixture(scope="module")
def lib():
    from view_fusion_amd import _lib
    return _lib.load()


def _fmt(kind):
    return "wino" if kind == 1 else "wino44"


# ------------------------------------------------------------------------------------------------ sizes
def test_restated_sizes_equal_the_library(lib):
    import ctypes
    nf, nb = ctypes.c_long(), ctypes.c_long()
    for Cout in GRID:
        for Cin in GRID:
            for KS in (1, 3):
                assert lib.vf_conv_pack_sizes(Cout, Cin, KS, ctypes.byref(nf), ctypes.byref(nb)) == 0
                assert (nf.value, nb.value) == pr.direct_sizes(Cout, Cin, KS), (Cout, Cin, KS)
            assert lib.vf_wino_pack_sizes(Cout, Cin, ctypes.byref(nf), ctypes.byref(nb)) == 0
            assert (nf.value, nb.value) == pr.wino_sizes(1, Cout, Cin), (Cout, Cin)
            assert lib.vf_wino44_pack_sizes(Cout, Cin, ctypes.byref(nf), ctypes.byref(nb)) == 0
            assert (nf.value, nb.value) == pr.wino_sizes(2, Cout, Cin), (Cout, Cin)
            assert lib.vf_conv_small_pack_floats(Cout, Cin) == pr.small_floats(Cout, Cin), (Cout, Cin)
            assert lib.vf_conv1x1_bf16x3_pack_dwords(Cout, Cin) == pr.b3_dwords(Cout, Cin), (Cout, Cin)
    assert lib.vf_conv_pack_sizes(8, 8, 5, ctypes.byref(nf), ctypes.byref(nb)) != 0


def test_restated_packs_have_the_restated_sizes_and_data_counts():
    for Cout, Cin in SHAPES:
        for bwd in (False, True):
            for KS in (1, 3):
                assert pr.direct_pack(pr.normal(Cout, Cin, KS, 1), bwd).size == pr.direct_sizes(Cout, Cin, KS)[bwd]
                assert pr.data_mask("direct", Cout, Cin, bwd, KS).sum() == Cout * Cin * KS * KS
            for kind in (1, 2):
                assert pr.wino_pack(pr.normal(Cout, Cin, 3, 1), kind, bwd).size == pr.wino_sizes(kind, Cout, Cin)[bwd]
                assert pr.data_mask(_fmt(kind), Cout, Cin, bwd).sum() == Cout * Cin * pr.WINO_SLICES[kind]
            M, K = (Cin, Cout) if bwd else (Cout, Cin)
            assert pr.b3_pack(pr.normal(Cout, Cin, 1, 1), bwd).size == 2 * pr.b3_dwords(M, K)
            assert pr.data_mask("bf16x3", Cout, Cin, bwd, 1).sum() == 3 * Cout * Cin
    for Cout, Cin in pr.SMALL_EDGES:
        assert pr.small_pack(pr.normal(Cout, Cin, 3, 1)).size == pr.small_floats(Cout, Cin)
        assert pr.data_mask("small", Cout, Cin).sum() == Cout * Cin * 9
    assert sorted(pr.F44_P.tolist()) == list(range(36))


# ------------------------------------------------------------------------------------------------ round trips
@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
def test_unpack_inverts_pack(bwd):
    for Cout, Cin in SHAPES + [(65, 33), (64, 32)]:
        for KS in (1, 3):
            w = pr.normal(Cout, Cin, KS, 2)
            assert np.array_equal(pr.direct_unpack(pr.direct_pack(w, bwd), Cout, Cin, KS, bwd), w)
        w1 = pr.normal(Cout, Cin, 1, 3)
        assert np.array_equal(pr.b3_unpack(pr.b3_pack(w1, bwd), Cout, Cin, bwd), w1)
        wl, wn = pr.lattice(Cout, Cin, 3, 4), pr.normal(Cout, Cin, 3, 5)
        for kind in (1, 2):
            # lattice weights: every tap is recovered exactly; any weights: the four corner taps (one stored value each)
            assert np.array_equal(pr.wino_unpack(pr.wino_pack_exact(wl, kind, bwd), kind, Cout, Cin, bwd), wl.astype(np.float64))
            got = pr.wino_unpack(pr.wino_pack(wn, kind, bwd).astype(np.float32), kind, Cout, Cin, bwd)
            assert np.array_equal(got[:, :, ::2, ::2], wn.astype(np.float64)[:, :, ::2, ::2])
    if not bwd:
        for Cout, Cin in pr.SMALL_EDGES:
            w = pr.normal(Cout, Cin, 3, 6)
            assert np.array_equal(pr.small_unpack(pr.small_pack(w), Cout, Cin), w)


def test_bf16_split_is_exact_and_round_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, -1.0 - 2.0 ** -8, 0.0], dtype=np.float32)
    assert pr.bf16_rne(x).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0xBF80, 0]          # ties go to the even mantissa
    w = pr.normal(64, 64, 1, 7).reshape(-1)
    p = pr.b3_split(w)
    assert np.array_equal(pr.bf16_value(p).astype(np.float64).sum(0), w.astype(np.float64))


# ------------------------------------------------------------------------------------------------ the rule
def test_lattice_weights_make_both_transforms_exact_in_any_precision():
    worst = 0
    for Cout, Cin in SHAPES:
        w = pr.lattice(Cout, Cin, 3, 8)
        for kind in (1, 2):
            for bwd in (False, True):
                exact = pr.wino_pack_exact(w, kind, bwd)
                mask = pr.data_mask(_fmt(kind), Cout, Cin, bwd)
                worst = max(worst, int(np.abs(exact).max() / 2.0 ** -16))
                for dtype in (np.float32, np.float64):
                    for values in (pr.wino_values, pr.wino_values_kernel_order):
                        got = pr.wino_layout(values(w, kind, bwd, dtype), kind).astype(np.float32)
                        assert pr.judge_bits(got, exact, mask, zero_sign=False)[0], (Cout, Cin, kind, bwd, dtype, values.__name__)
    # the largest stored integer (times 2^-16): 32 x 576 = 18432 for F(4x4) (slice (5, 5) = the tap itself), 3/2 of it for
    # the nested transform (slice (1, 5) = half the sum of three taps); far below 2^24 either way
    assert worst <= 27648


@pytest.mark.parametrize("kind", [1, 2], ids=["nested", "f44"])
def test_rule_separates_double_from_fp32_evaluation(kind):
    for Cout, Cin in SHAPES:
        w = pr.normal(Cout, Cin, 3, 9)
        for bwd in (False, True):
            r64 = pr.wino_pack(w, kind, bwd)
            mask, scale = pr.data_mask(_fmt(kind), Cout, Cin, bwd), pr.tap_max(w, kind, bwd)
            # accepted: the rounded reference itself, a double evaluation in another order, the rounded transposed product
            other = pr.wino_layout(pr.wino_values_kernel_order(w, kind, bwd, np.float64), kind).astype(np.float32)
            v = np.ascontiguousarray(pr._oriented(w, bwd)).astype(np.float64)
            rows = (pr.G2 * pr.NESTED_ROW_SIGN[:, None]) if kind == 1 else pr.G4
            third = pr.wino_layout(np.einsum("mkaj,bj->mkab", np.einsum("ai,mkij->mkaj", rows, v), pr.G4), kind).astype(np.float32)
            for name, got in (("rounded r64", r64.astype(np.float32)), ("kernel order", other), ("rows then columns", third)):
                ok, value, why = pr.judge_wino(got, r64, mask, scale)
                assert ok and value <= 1.0, (name, Cout, Cin, bwd, value, why)
            # rejected: the same two evaluations in fp32
            for values in (pr.wino_values, pr.wino_values_kernel_order):
                got = pr.wino_layout(values(w, kind, bwd, np.float32), kind).astype(np.float32)
                ok, value, why = pr.judge_wino(got, r64, mask, scale)
                assert not ok and value > 1.0, (values.__name__, Cout, Cin, bwd, value)
                frac = int(why.split()[0]) / mask.sum()
                assert frac > 0.2, (values.__name__, frac)             # (a third of the values, not a stray one)


def _wrong_layouts(p, mask, groups):
    """Layout mistakes applied to a correct pack `p` of [tile][chunk][group][64][8]: name -> pack."""
    out = {}
    a = p.reshape(-1, groups, 64 * 8).copy()
    a[:, [1, 2]] = a[:, [2, 1]]
    out["two exchanged groups"] = a.reshape(-1)
    out["a shifted chunk"] = np.roll(p.reshape(-1, groups * 64 * 8), 1, axis=0).reshape(-1)
    b = p.copy()
    b[int(np.argmin(mask))] = 1e-30
    out["a non-zero padding element"] = b
    return out


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
def test_rule_rejects_layout_mistakes(bwd):
    Cout, Cin = 65, 9                                      # two tiles / chunks in each direction, both partial
    for kind in (1, 2):
        ns = pr.WINO_SLICES[kind]
        mask = pr.data_mask(_fmt(kind), Cout, Cin, bwd)
        wl, wn = pr.lattice(Cout, Cin, 3, 10), pr.normal(Cout, Cin, 3, 11)
        exact, r64, scale = pr.wino_pack_exact(wl, kind, bwd), pr.wino_pack(wn, kind, bwd), pr.tap_max(wn, kind, bwd)
        assert pr.judge_bits(exact, exact, mask, zero_sign=False)[0] and pr.judge_wino(r64.astype(np.float32), r64, mask, scale)[0]
        wrong_l, wrong_n = _wrong_layouts(exact, mask, ns), _wrong_layouts(r64.astype(np.float32), mask, ns)
        if bwd:                                            # the backward pack of the UNROTATED kernel
            flip = lambda w: np.ascontiguousarray(w[:, :, ::-1, ::-1])
            wrong_l["unreversed taps"] = pr.wino_pack_exact(flip(wl), kind, True)
            wrong_n["unreversed taps"] = pr.wino_pack(flip(wn), kind, True).astype(np.float32)
        neg = exact.reshape(-1, ns, 512).copy()
        rows3 = [6 * 3 + b for b in range(6)] if kind == 1 else []
        neg[:, rows3] *= -1
        if kind == 1:
            wrong_l["row 3 not negated"] = neg.reshape(-1)
        for name in wrong_l:
            assert not pr.judge_bits(wrong_l[name], exact, mask, zero_sign=False)[0], (kind, name)
        for name in wrong_n:
            assert not pr.judge_wino(wrong_n[name], r64, mask, scale)[0], (kind, name)
        nan = r64.astype(np.float32)
        nan[0] = np.inf
        assert not pr.judge_wino(nan, r64, mask, scale)[0]
    for KS, groups in ((3, 9), (1, 4)):
        Co, Ci = (65, 9) if KS == 3 else (65, 33)
        w = pr.normal(Co, Ci, KS, 12)
        want, mask = pr.direct_pack(w, bwd), pr.data_mask("direct", Co, Ci, bwd, KS)
        assert pr.judge_bits(want, want, mask)[0]
        wrong = _wrong_layouts(want, mask, groups)
        if bwd and KS == 3:
            wrong["unreversed taps"] = pr.direct_pack(np.ascontiguousarray(w[:, :, ::-1, ::-1]), True)
        for name, got in wrong.items():
            assert not pr.judge_bits(got, want, mask)[0], (KS, name)
    # padding of either sign is zero; bf16 planes: a flipped last bit of the third plane, padding, a NaN
    w = pr.normal(65, 33, 1, 13)
    want, mask = pr.b3_pack(w, bwd), pr.data_mask("bf16x3", 65, 33, bwd, 1)
    minus = want.copy()
    minus[~mask] = 0x8000
    assert pr.judge_bits(want, want, mask)[0] and pr.judge_bits(minus, want, mask)[0]
    for at, val in ((int(np.argmax(mask)) + 2 * 512, None), (int(np.argmin(mask)), 1), (0, 0x7FC0)):
        bad = want.copy()
        bad[at] = bad[at] ^ 1 if val is None else val
        assert not pr.judge_bits(bad, want, mask)[0], (at, val)
    want = pr.small_pack(pr.normal(17, 96, 3, 14))
    mask = pr.data_mask("small", 17, 96)
    pad = want.copy()
    pad[int(np.argmin(mask))] = -0.0
    assert pr.judge_bits(pad, want, mask)[0]
    pad[int(np.argmin(mask))] = 1e-38
    assert not pr.judge_bits(pad, want, mask)[0]


# ------------------------------------------------------------------------------------------------ pack_all's tables
def test_pack_rows_of_the_three_launches():
    from view_fusion_amd import ops
    rng = np.random.default_rng(15)
    shapes = [(int(co), int(ci), 3 if k else int(rng.choice([1, 3]))) for co, ci, k in
              zip(rng.integers(1, 300, 40), rng.integers(1, 300, 40), rng.integers(0, 3, 40))]
    kinds = [int(k) for k in rng.integers(0, 3, 40)]
    shapes = [(co, ci, 3 if k else ks) for (co, ci, ks), k in zip(shapes, kinds)]
    ptrs = [(1000 + 3 * i, 1001 + 3 * i, 1002 + 3 * i) for i in range(40)]
    rows, totals = ops._pack_rows(shapes, kinds, ptrs)
    assert sum(len(r) for r in rows) == 40 and all(len(rows[k]) == kinds.count(k) for k in (0, 1, 2))
    for k in (0, 1, 2):
        mine = [i for i in range(40) if kinds[i] == k]
        unit = (1, 48, 72)[k]                              # 256-output units per workgroup of the launch
        first = 0
        for i, row in zip(mine, rows[k]):
            Cout, Cin, KS = shapes[i]
            nf, nb = pr.direct_sizes(Cout, Cin, KS) if k == 0 else pr.wino_sizes(k, Cout, Cin)
            want = list(ptrs[i]) + [Cout, Cin] + ([KS] if k == 0 else []) + [nf, nb, first]
            assert row == want, (k, i, row, want)
            assert (nf + nb) % 256 == 0 and first % unit == 0 and ((nf + nb) // 256) % unit == 0
            first += (nf + nb) // 256
        firsts = [r[-1] for r in rows[k]]
        assert all(b > a for a, b in zip(firsts, firsts[1:])) and firsts[0] == 0           # strictly increasing
        assert totals[k] == first == sum((r[-3] + r[-2]) // 256 for r in rows[k])
    assert ops._pack_rows([], []) == (([], [], []), (0, 0, 0))
    assert ops._pack_rows([(5, 7, 3)], [1])[0][1] == [[0, 0, 0, 5, 7] + list(pr.wino_sizes(1, 5, 7)) + [0]]


class _Tree(torch.nn.Module):
    def __init__(self, shapes):
        super().__init__()
        self.convs = torch.nn.ModuleList(torch.nn.Conv2d(ci, co, ks, padding=ks // 2) for co, ci, ks in shapes)
        for c in self.convs:
            object.__setattr__(c, "_vf_geom", (0, "same"))


@pytest.fixture
def host_pack_all(monkeypatch):
    """ops.pack_all with its launches recorded instead of made (CPU tensors): -> (run, launches)."""
    import ctypes
    from view_fusion_amd import ops
    launches = []
    monkeypatch.setattr(ops.packing, "_check", lambda *t: None)
    monkeypatch.setattr(ops.packing, "_stream", lambda: None)
    monkeypatch.setattr(ops.packing, "_call", lambda name, *a: launches.append((name,) + tuple(
        v.value if isinstance(v, ctypes.c_void_p) else v for v in a)))
    kinds = {}
    monkeypatch.setattr(ops.packing, "wino_kind", lambda S, Cin, Cout, H, W, KS, m, train=None: kinds.get((Cin, Cout), 0) if KS == 3 else 0)
    return ops, launches, kinds


def test_pack_all_launch_arguments_and_cache_rules_on_the_host(host_pack_all):
    ops, launches, kinds = host_pack_all
    shapes = [(65, 9, 3), (8, 16, 3), (6, 6, 1), (16, 8, 3), (40, 24, 3), (63, 7, 1), (24, 40, 3)]
    kinds.update({(9, 65): 1, (16, 8): 2, (8, 16): 1, (24, 40): 2, (40, 24): 0})
    want_kinds = [1, 2, 0, 1, 2, 0, 0]
    net = _Tree(shapes)
    for c in net.convs:                                    # stale inference caches of every format must lose their keys
        for attr in ("_vf_pack", "_vf_wpack", "_vf_w4pack"):
            object.__setattr__(c, attr, (("key",), torch.empty(1), torch.empty(1)))
        c.weight._vf_small_pack = (("key",), torch.empty(1))
    ops.pack_all(net, S=4, hw=(8, 8))
    layers, key, descs = net._vf_pack_plan
    ptrs = []
    for c, kind in zip(net.convs, want_kinds):
        attrs = ("_vf_pack", "_vf_wpack", "_vf_w4pack")
        for k, attr in enumerate(attrs):
            assert getattr(c, attr)[0] is None, attr
            assert getattr(c, attr + "_fresh", False) == (k == kind)
        assert c.weight._vf_small_pack[0] is None
        pf, pb = getattr(c, attrs[kind])[1:]
        Cout, Cin, KS, _ = c.weight.shape
        assert (pf.numel(), pb.numel()) == (pr.direct_sizes(Cout, Cin, KS) if kind == 0 else pr.wino_sizes(kind, Cout, Cin))
        ptrs.append((c.weight.data_ptr(), pf.data_ptr(), pb.data_ptr()))
    rows, totals = ops._pack_rows(shapes, want_kinds, ptrs)
    names = ("vf_conv_pack_weights_multi", "vf_wino_pack_weights_multi", "vf_wino44_pack_weights_multi")
    assert [l[0] for l in launches] == list(names)
    for k, (name, table, n, blk, stream) in enumerate(launches):
        assert descs[k][0].tolist() == rows[k] and table == descs[k][0].data_ptr()
        assert n == len(rows[k]) == descs[k][1] and blk == totals[k] == descs[k][2]        # the last argument = the table's total
    # the second call: same tables; a moved parameter or a changed kind: rebuilt
    ops.pack_all(net, S=4, hw=(8, 8))
    assert net._vf_pack_plan[2] is descs and [l[1] for l in launches[3:]] == [l[1] for l in launches[:3]]
    with torch.no_grad():
        net.convs[2].weight.data.mul_(2.0)                 # (in place: nothing moved)
    ops.pack_all(net, S=4, hw=(8, 8))
    assert net._vf_pack_plan[2] is descs
    net.convs[2].weight.data = net.convs[2].weight.data.clone()
    ops.pack_all(net, S=4, hw=(8, 8))
    moved = net._vf_pack_plan[2]
    assert moved is not descs and moved[0][0][0, 0].item() == net.convs[2].weight.data_ptr()
    kinds[(24, 40)] = 0                                    # layer 4 (Cin 24 -> Cout 40) leaves F(4x4) for the direct kernel
    ops.pack_all(net, S=4, hw=(8, 8))
    assert net._vf_pack_plan[2] is not moved and net._vf_pack_plan[2][0][1] == 4 and net._vf_pack_plan[2][2][1] == 1
    assert getattr(net.convs[4], "_vf_pack_fresh") and net.convs[4]._vf_pack[1].numel() == pr.direct_sizes(40, 24, 3)[0]
    # without S / a size every layer takes the direct format; no conv layer: no launch
    del launches[:]
    ops.pack_all(net)
    assert [l[0] for l in launches] == ["vf_conv_pack_weights_multi"] and launches[0][2] == 7
    del launches[:]
    ops.pack_all(torch.nn.Linear(3, 3))
    assert launches == []
