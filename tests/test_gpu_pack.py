"""Every packed-weight format and the grouped pack launches on a real MI355X, against tests/pack_ref.py.

(a) the single-layer entry points (vf_conv_pack_weights 3x3 and 1x1, vf_wino_pack_weights, vf_wino44_pack_weights,
    vf_conv_small_pack, vf_conv1x1_bf16x3_pack) at the padding edges -- Cout around the 64-row tile, Cin around the 8- / 32-
    channel chunk -- on NaN-filled buffers with a NaN guard of 4096 floats behind each: every element written, the guard
    untouched, a second launch bit-identical, w_bwd = NULL writes the forward pack only;
(b) one grouped launch (vf_conv_pack_weights_multi, vf_wino_pack_weights_multi, vf_wino44_pack_weights_multi; the table of
    ops._pack_rows, as pack_all builds it) bit-identical to the single launches, eight layers, a padded one first and last,
    the smallest possible one between two multi-tile ones;
(c) ops.pack_all on a small module tree: three launches, every layer's buffers equal to its single-layer pack, the table
    reused after a raw weight update and rebuilt after a parameter moved or a kind changed; per kind, at the smallest S at
    which the policy itself chooses it: the training conv2d behind pack_all launches no pack kernel, a second call of the
    same layer re-packs with the single launch, and after pack_all plus a raw update a no-grad conv2d re-packs and matches
    float64 on the CURRENT weights (cond_ref.judge at the route's own tolerance).

The rule is pack_ref's: direct, small and bf16x3 bit-identical to the restatement; Winograd on lattice weights bit-identical
to the exact integer result; Winograd on standard normal weights |got - r64| <= half_ulp32(r64) + 2^-45 max|taps|; padding
equal to zero; any non-finite value fails.  Measured values: profiles/pack_formats.md."""
import ctypes

import numpy as np
import pytest
import torch

import cond_ref as cr
import conv_plan_ref as cp
import pack_ref as pr
import wino_plan_ref as wp

pytestmark = pytest.mark.gpu

GUARD = 4096
NAN = float("nan")
_SINGLE = {0: "vf_conv_pack_weights", 1: "vf_wino_pack_weights", 2: "vf_wino44_pack_weights"}
_MULTI = {0: "vf_conv_pack_weights_multi", 1: "vf_wino_pack_weights_multi", 2: "vf_wino44_pack_weights_multi"}
_FMT = {1: "wino", 2: "wino44"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from view_fusion_amd import ops
    return ops._lib.load()


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    from view_fusion_amd.ops.core import _stream
    return _stream()


def _guarded(dev, n, words=False):
    """n NaN floats (words: n all-ones dwords = two bf16 NaNs each) with a guard of the same filling behind them."""
    buf = torch.full((n + GUARD,), -1, dtype=torch.int32, device=dev) if words else torch.full((n + GUARD,), NAN, device=dev)
    return buf[:n], buf


def _written(buf, n, what):
    if buf.dtype == torch.int32:
        assert bool((buf[n:] == -1).all()), f"written behind {what}"
        assert not bool((buf[:n].view(torch.int16) == -1).any()), f"{what} not fully written"
    else:
        assert bool(torch.isnan(buf[n:]).all()), f"written behind {what}"
        assert not bool(torch.isnan(buf[:n]).any()), f"{what} not fully written"


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _np(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int32 else a


def _sizes(fmt, Cout, Cin, KS):
    if fmt == "direct":
        return pr.direct_sizes(Cout, Cin, KS)
    if fmt == "bf16x3":
        return pr.b3_dwords(Cout, Cin), pr.b3_dwords(Cin, Cout)
    return pr.wino_sizes(1 if fmt == "wino" else 2, Cout, Cin)


def _single(lib, dev, fmt, w, with_bwd=True):
    """One single-layer launch of format `fmt` on fresh guarded buffers -> (fwd, bwd | None)."""
    Cout, Cin, KS, _ = w.shape
    nf, nb = _sizes(fmt, Cout, Cin, KS)
    words = fmt == "bf16x3"
    pf, bf = _guarded(dev, nf, words)
    pb, bb = _guarded(dev, nb, words) if with_bwd else (None, None)
    if fmt == "direct":
        rc = lib.vf_conv_pack_weights(_P(w), _P(pf), _P(pb), Cout, Cin, KS, _stream())
    elif fmt == "bf16x3":
        rc = lib.vf_conv1x1_bf16x3_pack(_P(w), _P(pf), _P(pb), Cout, Cin, _stream())
    else:
        rc = getattr(lib, _SINGLE[1 if fmt == "wino" else 2])(_P(w), _P(pf), _P(pb), Cout, Cin, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    _written(bf, nf, f"the forward {fmt} pack")
    if with_bwd:
        _written(bb, nb, f"the backward {fmt} pack")
    return pf, pb


def _judge(fmt, kind_of_w, w, got, bwd):
    """-> (passes, value, why) of one pack against the restatement."""
    Cout, Cin, KS, _ = w.shape
    mask = pr.data_mask(fmt, Cout, Cin, bwd, KS)
    if fmt == "direct":
        return pr.judge_bits(got, pr.direct_pack(w, bwd), mask)
    if fmt == "bf16x3":
        return pr.judge_bits(got, pr.b3_pack(w, bwd), mask)
    kind = 1 if fmt == "wino" else 2
    if kind_of_w == "lattice":
        return pr.judge_bits(got, pr.wino_pack_exact(w, kind, bwd), mask, zero_sign=False)
    return pr.judge_wino(got, pr.wino_pack(w, kind, bwd), mask, pr.tap_max(w, kind, bwd))


# ------------------------------------------------------------------------------------------------ (a) single layers
_CASES_A = ([("direct", 3, s) for s in pr.EDGES] + [("direct", 1, s) for s in pr.EDGES_1X1] + [("wino", 3, s) for s in pr.EDGES]
            + [("wino44", 3, s) for s in pr.EDGES] + [("bf16x3", 1, s) for s in pr.EDGES_1X1])


@pytest.mark.parametrize("fmt,KS,shape", _CASES_A, ids=[f"{f}-{k}x{k}-{s[0]}x{s[1]}" for f, k, s in _CASES_A])
def test_single_layer_pack_equals_the_restatement(dev, lib, fmt, KS, shape):
    Cout, Cin = shape
    bad = []
    print()
    for name, w in (("lattice", pr.lattice(Cout, Cin, KS, 21)), ("normal", pr.normal(Cout, Cin, KS, 22))):
        wd = torch.from_numpy(w).to(dev)
        pf, pb = _single(lib, dev, fmt, wd)
        pf2, pb2 = _single(lib, dev, fmt, wd)
        assert _same_bits(pf, pf2) and _same_bits(pb, pb2), "a second launch differs"
        pf3, _ = _single(lib, dev, fmt, wd, with_bwd=False)
        assert _same_bits(pf, pf3), "the forward pack differs without a backward pack"
        for bwd, p in ((False, pf), (True, pb)):
            ok, value, why = _judge(fmt, name, w, _np(p), bwd)
            print(f"PACK | {fmt} {KS}x{KS} | Cout {Cout} Cin {Cin} | {name} | {'bwd' if bwd else 'fwd'} | {p.numel()} | "
                  f"value {value:.8f} | {why} | {'ok' if ok else 'FAIL'}")
            if not ok:
                bad.append((name, bwd, value, why))
    assert not bad, bad


@pytest.mark.parametrize("Cout,Cin", pr.SMALL_EDGES, ids=[f"{co}x{ci}" for co, ci in pr.SMALL_EDGES])
def test_small_pack_equals_the_restatement(dev, lib, Cout, Cin):
    assert lib.vf_conv_small_supported(Cin, Cout, 16, 16, 3, 0) == 1
    w = pr.normal(Cout, Cin, 3, 23)
    wd = torch.from_numpy(w).to(dev)
    n = lib.vf_conv_small_pack_floats(Cout, Cin)
    assert n == pr.small_floats(Cout, Cin)
    got = []
    for _ in range(2):
        p, buf = _guarded(dev, n)
        assert lib.vf_conv_small_pack(_P(wd), _P(p), Cout, Cin, _stream()) == 0
        torch.cuda.synchronize()
        _written(buf, n, "the small pack")
        got.append(p)
    assert _same_bits(*got), "a second launch differs"
    ok, value, why = pr.judge_bits(_np(got[0]), pr.small_pack(w), pr.data_mask("small", Cout, Cin))
    print(f"\nPACK | small 3x3 | Cout {Cout} Cin {Cin} | normal | fwd | {n} | value {value:.8f} | {why} | {'ok' if ok else 'FAIL'}")
    assert ok, why
    assert np.array_equal(pr.small_unpack(_np(got[0]), Cout, Cin), w)


# ------------------------------------------------------------------------------------------------ (b) grouped launches
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["direct", "nested", "f44"])
def test_grouped_launch_equals_the_single_launches(dev, lib, kind):
    from view_fusion_amd import ops
    shapes = pr.MULTI_DIRECT if kind == 0 else [(co, ci, 3) for co, ci in pr.MULTI_3X3]
    fmt = "direct" if kind == 0 else _FMT[kind]
    ws = [torch.from_numpy(pr.normal(co, ci, ks, 30 + i)).to(dev) for i, (co, ci, ks) in enumerate(shapes)]
    singles = [_single(lib, dev, fmt, w) for w in ws]
    bufs = [(_guarded(dev, s[0].numel()), _guarded(dev, s[1].numel())) for s in singles]
    ptrs = [(w.data_ptr(), f[0].data_ptr(), b[0].data_ptr()) for w, (f, b) in zip(ws, bufs)]
    rows, totals = ops._pack_rows(shapes, [kind] * len(shapes), ptrs)
    assert len(rows[kind]) == len(shapes) >= 7 and not any(rows[k] for k in (0, 1, 2) if k != kind)
    blocks = [(r[-3] + r[-2]) // 256 for r in rows[kind]]
    assert blocks[2] == min(blocks) and blocks[1] > blocks[2] < blocks[3]          # the smallest between two larger ones
    table = torch.tensor(rows[kind], dtype=torch.int64).to(dev)
    assert getattr(lib, _MULTI[kind])(_P(table), len(shapes), totals[kind], _stream()) == 0
    torch.cuda.synchronize()
    print()
    for i, ((f, b), (sf, sb)) in enumerate(zip(bufs, singles)):
        _written(f[1], sf.numel(), f"layer {i}'s forward pack")
        _written(b[1], sb.numel(), f"layer {i}'s backward pack")
        same = _same_bits(f[0], sf) and _same_bits(b[0], sb)
        print(f"PACK | {_MULTI[kind]} | layer {i} {shapes[i]} | first_block {rows[kind][i][-1]} | blocks {blocks[i]} | "
              f"{'bit-identical to the single launch' if same else 'DIFFERS'}")
        assert same, (i, shapes[i])
    # nothing to do: no launch, no error
    assert getattr(lib, _MULTI[kind])(_P(table), 0, totals[kind], _stream()) == 0
    assert getattr(lib, _MULTI[kind])(_P(table), len(shapes), 0, _stream()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ (c) ops.pack_all
class _Tree(torch.nn.Module):
    """Conv layers nested two deep, annotated like the UNet's (output = the input size >> level)."""

    def __init__(self, shapes):
        super().__init__()
        half = len(shapes) // 2
        mk = lambda part: torch.nn.ModuleList(torch.nn.Conv2d(ci, co, ks, padding=ks // 2) for co, ci, ks in part)
        self.down, self.up = mk(shapes[:half]), torch.nn.Sequential(*mk(shapes[half:]))
        self.convs = list(self.down) + list(self.up)
        for c in self.convs:
            object.__setattr__(c, "_vf_geom", (0, "same"))


def _logged(fn):
    from view_fusion_amd import ops
    ops.st.KERNEL_LOG = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, [e[5] for e in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None


def _layer_pack(layer, kind):
    c = getattr(layer, ("_vf_pack", "_vf_wpack", "_vf_w4pack")[kind])
    return c[1], c[2]


def _equals_single(lib, dev, layer, kind):
    pf, pb = _layer_pack(layer, kind)
    sf, sb = _single(lib, dev, "direct" if kind == 0 else _FMT[kind], layer.weight.detach())
    return pf.numel() == sf.numel() and pb.numel() == sb.numel() and _same_bits(pf, sf) and _same_bits(pb, sb)


def test_pack_all_on_a_tree_in_all_three_formats(dev, lib, monkeypatch):
    from view_fusion_amd import ops
    shapes = [(65, 9, 3), (8, 16, 3), (6, 6, 1), (16, 8, 3), (40, 24, 3), (63, 7, 1), (24, 40, 3)]
    kinds = {(9, 65): 1, (16, 8): 2, (8, 16): 1, (24, 40): 2}                # (Cin, Cout) -> kind; everything else direct
    want = [1, 2, 0, 1, 2, 0, 0]
    monkeypatch.setattr(ops.packing, "wino_kind", lambda S, Cin, Cout, H, W, KS, m, train=None: kinds.get((Cin, Cout), 0) if KS == 3 else 0)
    torch.manual_seed(40)
    net = _Tree(shapes).to(dev)
    _, names = _logged(lambda: ops.pack_all(net, S=4, hw=(8, 8)))
    assert names == [_MULTI[0], _MULTI[1], _MULTI[2]], names
    for c, k in zip(net.convs, want):
        assert getattr(c, ("_vf_pack", "_vf_wpack", "_vf_w4pack")[k] + "_fresh") and _equals_single(lib, dev, c, k), (tuple(c.weight.shape), k)
    tables = net._vf_pack_plan[2]
    # a raw in-place update (no version bump): same tables, new packs
    for c in net.convs:
        v = c.weight._version
        c.weight.data.mul_(-1.5).add_(0.25)
        assert c.weight._version == v
    old = [tuple(t.clone() for t in _layer_pack(c, k)) for c, k in zip(net.convs, want)]
    _, names = _logged(lambda: ops.pack_all(net, S=4, hw=(8, 8)))
    assert names == [_MULTI[0], _MULTI[1], _MULTI[2]] and net._vf_pack_plan[2] is tables
    for c, k, o in zip(net.convs, want, old):
        assert _equals_single(lib, dev, c, k) and not _same_bits(o[0], _layer_pack(c, k)[0]), (tuple(c.weight.shape), k)
    # a moved parameter: rebuilt, and the new address is packed
    net.convs[3].weight.data = net.convs[3].weight.data.clone().mul_(2.0)
    _, names = _logged(lambda: ops.pack_all(net, S=4, hw=(8, 8)))
    moved = net._vf_pack_plan[2]
    assert moved is not tables and len(names) == 3
    assert all(_equals_single(lib, dev, c, k) for c, k in zip(net.convs, want))
    # a changed kind: rebuilt, the layer lands in its new format
    kinds[(24, 40)] = 0
    want[4] = 0
    _, names = _logged(lambda: ops.pack_all(net, S=4, hw=(8, 8)))
    assert net._vf_pack_plan[2] is not moved and [t[1] for t in net._vf_pack_plan[2]] == [4, 2, 1] and len(names) == 3
    assert all(_equals_single(lib, dev, c, k) for c, k in zip(net.convs, want))
    assert net.convs[4]._vf_pack_fresh and net.convs[4]._vf_w4pack[0] is None


_ROUTE_TOL = {"vf_conv_fwd": cp.TOL, "vf_wino_conv_fwd": wp.TOL["nested"], "vf_wino44_conv_fwd": wp.TOL["f44"],
              "vf_conv_small": cr.TOL["small_h"], "vf_conv_small_gn": cr.TOL["small_h"]}
_PACKS = ("vf_conv_pack_weights", "vf_wino_pack_weights", "vf_wino44_pack_weights", "vf_conv_small_pack")


def _against_fp64(label, y, x, layer, route):
    """y of a no-grad conv2d against float64 on the layer's CURRENT weights, on the first and the last view."""
    views = sorted({0, x.shape[0] - 1})
    xv, w, b = x[views].cpu(), layer.weight.detach().cpu(), layer.bias.detach().cpu()
    r64 = torch.nn.functional.conv2d(xv.double(), w.double(), b.double(), padding=1)
    r32 = torch.nn.functional.conv2d(xv, w, b, padding=1)
    err, e, bound, ok = cr.judge(y[views], r64, r32, _ROUTE_TOL[route])
    print(f"PACK | {label} | {route} | e {e:.3e} | err {err:.3e} | bound {bound:.3e} | ratio {err / bound:.3f} | {'ok' if ok else 'FAIL'}")
    return ok, (err, bound)


@pytest.mark.parametrize("kind,H,C", [(0, 16, 64), (1, 64, 64), (2, 64, 64)], ids=["direct", "nested", "f44"])
def test_pack_all_at_the_policys_own_choice(dev, lib, kind, H, C):
    """The smallest S at which ops.wino_kind itself takes `kind` for a C -> C 3x3 layer on an H x H map in training."""
    from view_fusion_amd import ops
    S = next((S for S in range(1, 129) if ops.wino_kind(S, C, C, H, H, 3, 0, train=True) == kind), None)
    assert S is not None, "the policy never chooses this kind here"
    torch.manual_seed(41 + kind)
    net = _Tree([(C, C, 3), (C, C, 1)]).to(dev)
    layer, other = net.convs
    x = torch.randn(S, C, H, H, device=dev)
    conv_name = "vf_conv_fwd" if kind == 0 else ops._WINO_ABI[kind][3]
    print()
    # inference first: a cached pack with a valid key (a second call is a cache hit)
    with torch.no_grad():
        y, names = _logged(lambda: ops.conv2d(x, layer))
        route = [n for n in names if n in _ROUTE_TOL]
        assert len(route) == 1 and [n for n in names if n in _PACKS], names
        ok, why = _against_fp64(f"kind {kind} S {S} {H}x{H} C {C} | no-grad, first", y, x, layer, route[0])
        assert ok, why
        _, names = _logged(lambda: ops.conv2d(x, layer))
        assert names == route, names
    if kind == 0:
        assert route == ["vf_conv_small_gn"] and layer.weight._vf_small_pack[0] is not None      # (the _vf_small_pack rule below)
    # pack_all: one launch per format present, the layer's buffers equal its single-layer pack
    _, names = _logged(lambda: ops.pack_all(net, S=S, hw=(H, H)))
    assert names == ([_MULTI[0]] if kind == 0 else [_MULTI[0], _MULTI[kind]]), names
    assert _equals_single(lib, dev, layer, kind) and _equals_single(lib, dev, other, 0)
    assert getattr(layer.weight, "_vf_small_pack", (None,))[0] is None
    # the training conv2d of this forward consumes the fresh pack; a second call of the layer re-packs with the single launch
    with torch.enable_grad():
        y1, names = _logged(lambda: ops.conv2d(x, layer))
        assert names == [conv_name], names
        y2, names = _logged(lambda: ops.conv2d(x, layer))
        assert names == [_SINGLE[kind], conv_name], names
        assert y1.requires_grad and torch.equal(y1, y2)
    # pack_all + a raw update: the no-grad forward must re-pack, whatever format its route reads
    ops.pack_all(net, S=S, hw=(H, H))
    v = layer.weight._version
    layer.weight.data.mul_(-1.5).add_(0.125)
    assert layer.weight._version == v
    with torch.no_grad():
        y, names = _logged(lambda: ops.conv2d(x, layer))
        assert [n for n in names if n in _ROUTE_TOL] == route and len([n for n in names if n in _PACKS]) == 1, names
        ok, why = _against_fp64(f"kind {kind} S {S} {H}x{H} C {C} | no-grad after pack_all + raw update", y, x, layer, route[0])
        assert ok, why
