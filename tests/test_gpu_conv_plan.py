"""Every reachable plan of the direct (non-Winograd) forward / dgrad convolution launchers on a real MI355X, against float64.

The cases come from tests/conv_plan_ref.py:cases() -- per launcher (conv_mfma_kernel, conv1x1_kernel<1>, conv_any_kernel)
the cheapest representative of every plan class: table row, tile size, views per tile, half-empty last tile, split of 1 /
2-8 / 9-15 / 16 ranges, even and uneven ranges, every pricing state (as priced / priced, fewer taken / priced, one taken),
channel padding, the SAFE instantiation, a concatenated input with its boundary on and inside a range, a split output,
the plain reduce whole and ragged, all six reduce + GroupNorm variants with full and clamped lanes, whole and partly filled
batches, with and without y, both GroupNorm fallbacks, the 1x1 kernel's thresholds from either side, the general kernel's
tile / split / partial-tile / square-power-of-two branches -- and the hand-written SPECIALS (mode 4 with a priced workspace,
the S = 21 / 22 pricing cases, the (8, 1024) variant, the bench step's layers).  tests/test_conv_plan_host.py checks on the
CPU that the restatement equals the library on the whole domain, that the list holds every class the SMALL / TINY layers
reach, and that the rule below rejects six wrong split decompositions.  conv1x1_kernel<2>'s natural grid costs 2.1e9
multiply-adds at the least: conv_plan_ref.over_cap_classes() names its classes, test_conv1x1_training_size_kernel runs it.

(a) parity per plan class through the C ABI entry the case names (vf_conv_fwd / vf_conv_fwd_gn / vf_conv1x1_cat_fwd /
vf_conv1x1_cat_dgrad: (d) of the issue), with every epilogue operand the entry takes and bare, the plan queried first
(vf_conv_fwd_plan) and asserted equal to the restatement; (b) NaN-filled outputs and workspace with NaN guards, twice,
bit-identical, exactly ks slabs written; (c) smaller workspaces; (e) through ops.conv2d / ops.conv2d_gn.

The rule (cond_ref.judge): err = max|a - r64| / max|r64| <= max(4 e, 2e-5), r64 = F.conv2d (conv_transpose2d for mode 4;
GroupNorm + Swish restated) in float64 on the CPU, e = stock fp32 CPU torch's error on the same inputs; any non-finite
value fails.  Measured values: profiles/conv_fwd_plan.md."""
import ctypes

import pytest
import torch

import cond_ref as cr
import conv_plan_ref as cp

pytestmark = pytest.mark.gpu

cp.check_env()

GUARD = 4096
NAN = float("nan")
_CORES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _refs(c, full):
    """(inputs, r64, r32) of a case; the convolution itself is computed once per shape and left unchanged."""
    t = cp.inputs(c)
    key = (c.S, c.Cin, c.Cout, c.H, c.W, c.KS, c.mode)
    if key not in _CORES:
        if len(_CORES) > 8:
            _CORES.clear()
        _CORES[key] = (cp.conv_core(t, c, torch.float64), cp.conv_core(t, c, torch.float32))
    k64, k32 = _CORES[key]
    return t, cp.conv_ref(t, c, torch.float64, full, k64), cp.conv_ref(t, c, torch.float32, full, k32)


def _query(lib, c, has_ws, ws_floats):
    out = (ctypes.c_int * 8)()
    rc = lib.vf_conv_fwd_plan(c.S, c.Cin, c.Cout, c.H, c.W, c.KS, c.mode, c.C1, c.C1o, c.gn, int(has_ws), int(ws_floats),
                              ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0
    return list(out)


def _label(c, d):
    return (f"{cp.case_id(c)} | {cp.entry(c)} | {cp.ROUTES[d['route']]} npt {d['npt']} nblk {d['nblk']} ks {d['ks']}"
            f"{' SAFE' if d['safe'] else ''}{' half' if d['half'] else ''} | {cp.RED_NAMES[d['reduce']]}"
            + (f" ({d['nv']}, {d['nt']})" if d["nv"] else ""))


def _judge_all(label, got, r64, r32):
    rows = [(n, *cr.judge(a, b, f, cp.TOL)) for n, a, b, f in zip(("y", "gn(y)"), got, r64, r32) if a is not None]
    print()
    for n, err, e, bound, ok in rows:
        print(f"CONVPLAN | {label} | {n} | e {e:.3e} | err {err:.3e} | bound {bound:.3e} | {'ok' if ok else 'FAIL'}")
    assert all(r[4] for r in rows), [(r[0], r[1], r[3]) for r in rows if not r[4]]


def _guarded(dev, *shape):
    """A NaN-filled tensor of `shape` with GUARD NaN floats behind it -> (view, whole buffer)."""
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + GUARD,), NAN, device=dev)
    return buf[:n].view(*shape), buf


class _Launch:
    """One case's device tensors, packed weights and its call through the C ABI."""

    def __init__(self, lib, dev, c, t):
        from view_fusion_amd.ops.core import _ptr, _stream
        self.lib, self.dev, self.c = lib, dev, c
        self.t = {k: v.to(dev).contiguous() for k, v in t.items()}
        w = self.t["w"]
        # mode 4 / a split output run a layer backwards: the dgrad pack of the layer whose dgrad is this call
        lw = w if c.mode == 4 else (w.transpose(0, 1).contiguous() if c.C1o else w)
        back = c.mode == 4 or bool(c.C1o)
        lo, li = lw.shape[0], lw.shape[1]
        nf, nb = ctypes.c_long(), ctypes.c_long()
        assert lib.vf_conv_pack_sizes(lo, li, c.KS, ctypes.byref(nf), ctypes.byref(nb)) == 0
        wf, wb = torch.empty(nf.value, device=dev), torch.empty(nb.value, device=dev)
        assert lib.vf_conv_pack_weights(_ptr(lw), _ptr(wf), _ptr(wb), lo, li, c.KS, _stream()) == 0
        self.wp = wb if back else wf
        x = self.t["x"]
        self.x1, self.x2 = (x[:, :c.C1].contiguous(), x[:, c.C1:].contiguous()) if c.C1 else (x, None)

    def outputs(self):
        """NaN-filled, guarded: [(y | (y1, y2)), a | None] and their whole buffers."""
        c = self.c
        Ho, Wo = cp.out_size(c)
        bufs = []
        if c.C1o:
            y1, b1 = _guarded(self.dev, c.S, c.C1o, Ho, Wo)
            y2, b2 = _guarded(self.dev, c.S, c.Cout - c.C1o, Ho, Wo)
            y, bufs = (y1, y2), [b1, b2]
        else:
            y, b = _guarded(self.dev, c.S, c.Cout, Ho, Wo)
            bufs = [b]
        a = None
        if c.gn:
            a, b = _guarded(self.dev, c.S, c.Cout, Ho, Wo)
            bufs.append(b)
        return y, a, bufs

    def workspace(self, floats):
        return torch.full((int(floats) + GUARD,), NAN, device=self.dev)

    def run(self, y, a, ws, ws_floats, full=True):
        from view_fusion_amd.ops.core import _ptr, _stream
        c, t = self.c, self.t
        b, v, r = cp.operands(c, full)
        bias, vbias, res = (t["bias"] if b else None), (t["vbias"] if v else None), (t["res"] if r else None)
        dims = (c.S, c.Cin, c.Cout, c.H, c.W)
        wsp, nws = (_ptr(ws), int(ws_floats)) if ws is not None else (None, 0)
        if c.C1:
            rc = self.lib.vf_conv1x1_cat_fwd(_ptr(self.x1), _ptr(self.x2), c.C1, _ptr(self.wp), _ptr(bias), _ptr(y), wsp, nws, *dims,
                                             _stream())
        elif c.C1o:       # (the entry names the layer's channels: Cin = this call's Cout and the other way round)
            rc = self.lib.vf_conv1x1_cat_dgrad(_ptr(self.x1), _ptr(self.wp), _ptr(y[0]), _ptr(y[1]), c.C1o, c.S, c.Cout, c.Cin,
                                               c.H, c.W, _stream())
        elif c.gn:
            stats = torch.empty(2 * c.S * c.gn, device=self.dev)
            rc = self.lib.vf_conv_fwd_gn(_ptr(self.x1), _ptr(self.wp), _ptr(bias), _ptr(vbias), _ptr(res), _ptr(y), c.store_y,
                                         _ptr(t["gamma"]), _ptr(t["beta"]), _ptr(a), _ptr(stats), c.gn, 1e-5, 1, wsp, nws, *dims,
                                         c.KS, c.mode, _stream())
        else:
            rc = self.lib.vf_conv_fwd(_ptr(self.x1), _ptr(self.wp), _ptr(bias), _ptr(vbias), _ptr(res), _ptr(y), wsp, nws, *dims,
                                      c.KS, c.mode, _stream())
        torch.cuda.synchronize()
        return rc


def _y_of(c, d, y):
    """The conv output where the call leaves one (store_y = 0 under reduce + GroupNorm: none)."""
    if c.C1o:
        return torch.cat(y, 1)
    return None if (c.gn and not c.store_y and d["reduce"] == cp.RED_GN) else y


# ------------------------------------------------------------------------------------------------ (a) + (d) parity per plan class
@pytest.mark.parametrize("c", cp.cases(), ids=cp.case_id)
def test_conv_plan_class_vs_fp64(dev, c):
    from view_fusion_amd import ops
    lib = ops._lib.load()
    d = cp.plan(c)
    need = lib.vf_conv_fwd_ws_floats(c.S, c.Cin, c.Cout, c.H, c.W, c.KS)
    assert need == d["need"] and (d["ks"] == 1 or d["ks"] * d["out_floats"] <= need)
    assert _query(lib, c, need > 0, need) == cp.fields(d), (cp.case_id(c), d)
    for full in (True, False):
        if not full and not any(cp.operands(c, True)):
            continue
        t, r64, r32 = _refs(c, full)
        L = _Launch(lib, dev, c, t)
        y, a, _ = L.outputs()
        ws = L.workspace(need) if need > 0 else None
        assert L.run(y, a, ws, need, full) == 0
        _judge_all(_label(c, d) + (" | all operands | " if full else " | bare | ") + c.why, [_y_of(c, d, y), a], r64, r32)


# ------------------------------------------------------------------------------------------------ (b) hygiene
@pytest.mark.parametrize("c", cp.hygiene_cases(), ids=cp.case_id)
def test_conv_writes_every_output_and_exactly_its_slabs(dev, c):
    """Outputs and workspace start as NaN with a NaN guard behind each: the result must be finite and right, exactly ks slabs
    of the workspace finite and every float beyond still NaN (ks = 1, mode 4 and a split output among them: untouched),
    y untouched where reduce + GroupNorm runs with store_y = 0, every guard untouched, a second launch bit-identical."""
    from view_fusion_amd import ops
    lib = ops._lib.load()
    d = cp.plan(c)
    t, r64, r32 = _refs(c, True)
    L = _Launch(lib, dev, c, t)
    need = max(d["need"], d["out_floats"])               # (a workspace is passed even where none is priced)
    dd = cp.plan(c, need)
    assert _query(lib, c, True, need) == cp.fields(dd) and dd["ks"] == d["ks"]
    runs = []
    for _ in range(2):
        y, a, bufs = L.outputs()
        ws = L.workspace(need)
        assert L.run(y, a, ws, need) == 0
        used = d["ks"] * d["out_floats"] if d["ks"] > 1 else 0
        assert bool(torch.isfinite(ws[:used]).all()), "a slab of the plan was not written"
        assert bool(torch.isnan(ws[used:]).all()), "written past the plan's slabs"
        for b in bufs:
            assert bool(torch.isnan(b[-GUARD:]).all()), "written past an output"
        yy = _y_of(c, d, y)
        if yy is None:
            assert bool(torch.isnan(y).all()), "store_y = 0: y must stay untouched"
        runs.append([yy, a])
    _judge_all(_label(c, d) + " | NaN-filled", runs[0], r64, r32)
    for p, q in zip(*runs):
        assert (p is None and q is None) or torch.equal(p, q)


# ------------------------------------------------------------------------------------------------ (c) smaller workspaces
@pytest.mark.parametrize("c", cp.clip_cases(), ids=cp.case_id)
def test_conv_with_a_smaller_workspace(dev, c):
    """A workspace below the priced size is a legal input: the launcher clamps ks to the slabs it holds (one slab, half the
    slabs, one float short of two slabs: one range; none: one range), as the restatement predicts, same result."""
    from view_fusion_amd import ops
    lib = ops._lib.load()
    full = cp.plan(c)
    assert full["ks"] >= 4
    t, r64, r32 = _refs(c, True)
    L = _Launch(lib, dev, c, t)
    slab = full["out_floats"]
    for name, floats, want in (("one slab", slab, 1), ("half the slabs", (full["ks"] + 1) // 2 * slab, (full["ks"] + 1) // 2),
                               ("one float short of two slabs", 2 * slab - 1, 1), ("no workspace", None, 1)):
        d = cp.plan(c, floats)
        assert d["ks"] == want and _query(lib, c, floats is not None, floats or 0) == cp.fields(d)
        y, a, bufs = L.outputs()
        ws = L.workspace(full["need"]) if floats is not None else None
        assert L.run(y, a, ws, floats or 0) == 0
        if ws is not None:
            used = d["ks"] * slab if d["ks"] > 1 else 0
            assert bool(torch.isfinite(ws[:used]).all()) and bool(torch.isnan(ws[used:]).all()), "slabs of the clamped plan"
        # (store_y = 0 leaves y only while the reduce + GroupNorm launch runs: with one range the conv writes y itself)
        _judge_all(_label(c, d) + f" | ws = {name}", [_y_of(c, d, y), a], r64, r32)


# ------------------------------------------------------------------------------------------------ (e) through ops
# (Cin, Cout, input map, KS, mode): the bench step's stride-2 and 1x1 layers (SMALL network)
OPS_LAYERS = ((64, 64, 64, 3, "down2"), (128, 128, 32, 3, "down2"), (192, 192, 16, 3, "down2"),
              (64, 128, 32, 1, "same"), (128, 192, 16, 1, "same"), (192, 320, 8, 1, "same"))
OPS_CASES = [(l, S) for l in OPS_LAYERS for S in (1, 6, 12)]      # (the sampler's view counts; at S = 96 these layers cost
#                                                                     3.6e9 multiply-adds: their plans run scaled in SPECIALS)


def _ops_case(layer, S, **kw):
    Cin, Cout, Hin, KS, mode = layer
    H = Hin // 2 if mode == "down2" else Hin
    return cp.mk(S, Cin, Cout, H, H, KS, {"same": 0, "down2": 1}[mode], **kw)


def _logged(fn):
    from view_fusion_amd import ops
    ops.st.KERNEL_LOG = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, [e[5] for e in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None


def _layer(dev, c, t):
    layer = torch.nn.Conv2d(c.Cin, c.Cout, c.KS, stride=2 if c.mode == 1 else 1, padding=c.KS // 2)
    with torch.no_grad():
        layer.weight.copy_(t["w"])
        layer.bias.copy_(t["bias"])
    return layer.to(dev)


@pytest.mark.parametrize("layer,S", OPS_CASES, ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else f"S{v}")
def test_conv_through_ops_forward_and_dgrad(dev, layer, S):
    """ops.conv2d with autograd on: the forward runs vf_conv_fwd with the plan the query reports for (Cin, Cout), the dgrad
    the same entry with Cin <-> Cout (stride 2: mode 4, no workspace) -- both under the rule against float64."""
    from view_fusion_amd import ops
    lib = ops._lib.load()
    c = _ops_case(layer, S)
    t = cp.inputs(c)
    mod = _layer(dev, c, t)
    x = t["x"].to(dev).requires_grad_(True)
    gy = cp.wp.rnd(c.S, c.Cout, c.H, c.W, seed=10)

    def step():
        y = ops.conv2d(x, mod, view_bias=t["vbias"].to(dev), residual=t["res"].to(dev), mode=layer[4])
        y.backward(gy.to(dev))
        return y.detach()
    y, names = _logged(step)
    assert [n for n in names if n.startswith("vf_conv") and "wgrad" not in n and "pack" not in n] == ["vf_conv_fwd", "vf_conv_fwd"], names
    d = cp.plan(c)
    assert _query(lib, c, d["need"] > 0, d["need"]) == cp.fields(d)
    back = cp.mk(S, c.Cout, c.Cin, c.H, c.W, c.KS, 4 if c.mode == 1 else 0)
    db = cp.plan(back, None if c.mode == 1 else "priced")
    assert _query(lib, back, c.mode != 1 and db["need"] > 0, db["need"] if c.mode != 1 else 0) == cp.fields(db)
    refs = []
    for dt in (torch.float64, torch.float32):
        xc = t["x"].to(dt).requires_grad_(True)
        yc = cp.conv_ref(dict(t, x=xc), c, dt)[0]
        yc.backward(gy.to(dt))
        refs.append([yc.detach(), xc.grad])
    label = f"{cp.case_id(c)} | ops.conv2d | fwd {cp.ROUTES[d['route']]} ks {d['ks']} | dgrad {cp.ROUTES[db['route']]} ks {db['ks']}"
    rows = [(n, *cr.judge(a, b, f, cp.TOL)) for n, a, b, f in zip(("y", "dx"), (y, x.grad), *refs)]
    print()
    for n, err, e, bound, ok in rows:
        print(f"CONVPLAN | {label} | {n} | e {e:.3e} | err {err:.3e} | bound {bound:.3e} | {'ok' if ok else 'FAIL'}")
    assert all(r[4] for r in rows), rows


@pytest.mark.parametrize("want_y", [False, True])
@pytest.mark.parametrize("layer,S", [(l, S) for l in OPS_LAYERS[:3] for S in (1, 6, 12)],
                         ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else f"S{v}")
def test_conv2d_gn_through_ops(dev, layer, S, want_y):
    """ops.conv2d_gn without autograd on the stride-2 layers (no Winograd, no one-launch kernel for them): vf_conv_fwd_gn
    wherever a workspace is priced, with the reduce the query reports; conv + GroupNorm launches otherwise."""
    from view_fusion_amd import ops
    lib = ops._lib.load()
    c = _ops_case(layer, S, gn=cp.GROUPS, store_y=int(want_y))
    t, r64, r32 = _refs(c, True)
    mod = _layer(dev, c, t)
    gn = torch.nn.GroupNorm(cp.GROUPS, c.Cout).to(dev)
    with torch.no_grad():
        gn.weight.copy_(t["gamma"])
        gn.bias.copy_(t["beta"])
        (y, a), names = _logged(lambda: ops.conv2d_gn(t["x"].to(dev), mod, gn, cp.GROUPS, True, view_bias=t["vbias"].to(dev),
                                                     residual=t["res"].to(dev), mode=layer[4], want_y=want_y))
    d = cp.plan(c)
    fused = d["need"] > 0
    assert ("vf_conv_fwd_gn" in names) == fused and ("vf_conv_fwd" in names) == (not fused), (names, d)
    assert _query(lib, c, fused, d["need"]) == cp.fields(d)
    assert (y is not None) == bool(want_y or not fused)
    _judge_all(_label(c, d) + " | ops.conv2d_gn", [y if want_y else None, a], r64, r32)
