"""Every reachable K-split tail plan of the two persistent Winograd kernels on a real MI355X, against float64.

The cases come from tests/wino_plan_ref.py:cases() -- per (kernel, map) the cheapest representative of every plan class
(split, last K range shorter than the others), the launches around the rounds of 256 workgroups (a split tail behind one
and behind two full rounds, three or more rounds with a ragged last one, more than 256 tail parts, one tail tile), the
upsampling load, a ragged last chunk under a split, and the nested kernel's second batch of partial loads on a ragged
group of 8x8 views.  tests/test_wino_plan_host.py checks on the CPU that the list holds every class the SMALL / TINY layers
reach and that the rule below rejects a K-split with a dropped chunk or a shifted range.

(a) forward + backward through ops.conv2d (bias, per-view bias, residual), kernel forced, route and plan class confirmed
    before the launch; (b) the C ABI on NaN-filled outputs and workspace with a NaN guard behind it, twice, bit-identical;
(c) the launchers' plain-grid fallback (no workspace / one float short); (d) the GroupNorm evaluated by the fix-up launch.

The rule (cond_ref.judge): err = max|a - r64| / max|r64| <= max(4 e, tol), r64 = F.conv2d in float64 on the CPU, e = stock
fp32 CPU torch's error on the same inputs, tol = 2e-5 (nested) / 3e-5 (F(4x4)) for y and dx, 1e-4 for dW, 2e-5 for the bias
gradients, 1e-6 for d(residual); any non-finite value fails.  Measured values: profiles/wino_tail_plan.md."""
import ctypes

import pytest
import torch

import cond_ref as cr
import wino_plan_ref as wp

pytestmark = pytest.mark.gpu

wp.check_env()

FORCE = {"nested": "FORCE_WINOGRAD", "f44": "FORCE_WINOGRAD44"}
ABI = {"nested": ("vf_wino_pack_sizes", "vf_wino_pack_weights", "vf_wino_conv_fwd", "vf_wino_conv_ws_floats", "vf_wino_conv_fill_pct"),
       "f44": ("vf_wino44_pack_sizes", "vf_wino44_pack_weights", "vf_wino44_conv_fwd", "vf_wino44_conv_ws_floats",
               "vf_wino44_conv_fill_pct")}
GUARD = 4096
_REFS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _refs(c, backward=True):
    """(inputs, r64, r32) of a case, computed once and left unchanged."""
    key = (c.S, c.Cin, c.Cout, c.H, c.mode, backward)
    if key not in _REFS:
        if len(_REFS) > 4:
            _REFS.clear()
        t = wp.inputs(c)
        _REFS[key] = (t, wp.conv_ref(t, c.mode, torch.float64, backward), wp.conv_ref(t, c.mode, torch.float32, backward))
    return _REFS[key]


def _label(c, d):
    return (f"{c.kernel} {c.H}x{c.H} {c.mode} S={c.S} {c.Cin}->{c.Cout} | T {d['T']} nfull {d['nfull']} split {d['split']} "
            f"per {d['per']} last {d['last']} parts {d['parts']}")


def _judge_all(label, names, got, r64, r32, tols):
    rows = [(n, *cr.judge(a, b, c, t)) for n, a, b, c, t in zip(names, got, r64, r32, tols)]
    print()
    for n, d, e, b, ok in rows:
        print(f"TAIL | {label} | {n} | e {e:.3e} | err {d:.3e} | bound {b:.3e} | {'ok' if ok else 'FAIL'}")
    assert all(r[4] for r in rows), [(r[0], r[1], r[3]) for r in rows if not r[4]]


def _confirm_plan(lib, c, ws=None):
    """The library's own host functions give this launch the plan the case list claims -- vf_wino_conv_plan, the function
    the launcher executes, included: describe()'s plan with the workspace the launch asks for (ws = None), the plain grid
    with the (has_ws, floats) a fallback case passes."""
    d = wp.describe(c.kernel, c.S, c.Cin, c.Cout, c.H, c.H)
    tiles = ctypes.c_int(0)
    getattr(lib, ABI[c.kernel][4])(c.S, c.Cin, c.Cout, c.H, c.H, ctypes.byref(tiles))
    need = getattr(lib, ABI[c.kernel][3])(c.S, c.Cin, c.Cout, c.H, c.H)
    assert tiles.value == d["T"] and need == d["parts"] * wp.PART_FLOATS[c.kernel], (wp.case_id(c), d, tiles.value, need)
    has_ws, nws = (1, need) if ws is None else ws
    out = (ctypes.c_int * 8)()
    rc = lib.vf_wino_conv_plan(wp.KIND[c.kernel], c.S, c.Cin, c.Cout, c.H, c.H, {"same": 0, "up2": 2}[c.mode], has_ws, nws,
                               ctypes.cast(out, ctypes.c_void_p))
    plan = dict(zip(wp.PLAN_FIELDS, out))
    assert rc == 0 and plan == wp.launch_plan(c.kernel, c.S, c.Cin, c.Cout, c.H, c.H, has_ws, nws), (wp.case_id(c), rc, plan)
    if has_ws and nws >= need:
        assert all(plan[k] == d[k] for k in ("T", "nch", "nfull", "split", "per")), (wp.case_id(c), d, plan)
    else:
        assert (plan["T"], plan["nch"], plan["nfull"], plan["split"], plan["fixup_grid"]) == (d["T"], d["nch"], d["T"], 1, 0), plan
    return d, need


# ------------------------------------------------------------------------------------------------ (a) parity per plan class
@pytest.mark.parametrize("c", wp.cases(), ids=wp.case_id)
def test_tail_plan_class_vs_fp64(dev, c):
    from view_fusion_amd import ops
    lib = ops._lib.load()
    m = ops._MODES[c.mode]
    d, _ = _confirm_plan(lib, c)
    t, r64, r32 = _refs(c)
    layer = torch.nn.Conv2d(c.Cin, c.Cout, 3, padding=1)
    with torch.no_grad():
        layer.weight.copy_(t["w"])
        layer.bias.copy_(t["b"])
    layer = layer.to(dev)
    xg, vbg, rg = (t[k].to(dev).requires_grad_(True) for k in ("x", "vb", "res"))
    setattr(ops.st, FORCE[c.kernel], True)
    ops.st.KERNEL_LOG = []
    try:
        assert ops.wino_kind(c.S, c.Cin, c.Cout, c.H, c.H, 3, m, True) == (1 if c.kernel == "nested" else 2)
        y = ops.conv2d(xg, layer, view_bias=vbg, residual=rg, mode=c.mode)
        y.backward(t["gy"].to(dev))
        torch.cuda.synchronize()
        log = [(e[0], e[5]) for e in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None
        setattr(ops.st, FORCE[c.kernel], False)
    assert log.count(("conv_fwd", wp.ENTRY[c.kernel])) == 1 and log.count(("conv_dgrad", wp.ENTRY[c.kernel])) == 1, log
    got = [y, xg.grad, layer.weight.grad, layer.bias.grad, vbg.grad, rg.grad]
    _judge_all(_label(c, d) + " | " + c.why, wp.NAMES, got, r64, r32, wp.tols(c.kernel))


# ------------------------------------------------------------------------------------------------ (b), (c) the C ABI
def _abi_launch(lib, dev, c, t, ws_mode):
    """One forward through the C ABI on a NaN-filled output.  ws_mode "guard": the workspace the launch asks for, NaN-filled,
    with GUARD NaN floats behind it; "null": no workspace; "short": one float less than asked for.
    -> (y, guard floats | None)."""
    from view_fusion_amd.ops import _ptr, _stream
    f_sizes, f_pack, f_conv = (getattr(lib, n) for n in ABI[c.kernel][:3])
    m = {"same": 0, "up2": 2}[c.mode]
    _, need = _confirm_plan(lib, c)
    nf, nb = ctypes.c_long(), ctypes.c_long()
    assert f_sizes(c.Cout, c.Cin, ctypes.byref(nf), ctypes.byref(nb)) == 0
    g = {k: t[k].to(dev).contiguous() for k in ("w", "b", "x", "vb", "res")}
    uf = torch.zeros(nf.value, device=dev)
    assert f_pack(_ptr(g["w"]), _ptr(uf), None, c.Cout, c.Cin, _stream()) == 0
    y = torch.full((c.S, c.Cout, c.H, c.H), float("nan"), device=dev)
    ws = torch.full((need + GUARD,), float("nan"), device=dev)
    wsp, nws = {"guard": (_ptr(ws), need), "null": (None, 0), "short": (_ptr(ws), need - 1)}[ws_mode]
    _confirm_plan(lib, c, (int(wsp is not None), nws))
    rc = f_conv(_ptr(g["x"]), _ptr(uf), _ptr(g["b"]), _ptr(g["vb"]), _ptr(g["res"]), _ptr(y), wsp, nws, c.S, c.Cin, c.Cout,
                c.H, c.H, m, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return y, ws[need:]


@pytest.mark.parametrize("c", wp.hygiene_cases(), ids=wp.case_id)
def test_tail_writes_every_output_and_stays_inside_its_workspace(dev, c):
    """Neither a tile that is never written nor a partial that is read before it is written can hide behind recycled
    memory here: y and the workspace start as NaN, the result must be finite and right, the guard untouched, and a second
    launch bit-identical."""
    from view_fusion_amd import ops
    lib = ops._lib.load()
    d = wp.describe(c.kernel, c.S, c.Cin, c.Cout, c.H, c.H)
    t, r64, r32 = _refs(c, backward=False)
    y1, guard1 = _abi_launch(lib, dev, c, t, "guard")
    y2, guard2 = _abi_launch(lib, dev, c, t, "guard")
    assert bool(torch.isnan(guard1).all()) and bool(torch.isnan(guard2).all())
    _judge_all(_label(c, d) + " | C ABI on NaN", ("y",), [y1], r64, r32, (wp.TOL[c.kernel],))
    assert torch.equal(y1, y2)


@pytest.mark.parametrize("ws_mode", ["null", "short"])
@pytest.mark.parametrize("c", [c for c in wp.hygiene_cases() if wp.describe(c.kernel, c.S, c.Cin, c.Cout, c.H, c.H)["split"] > 1],
                         ids=wp.case_id)
def test_tail_without_room_runs_the_plain_grid(dev, c, ws_mode):
    """No workspace, or one float too few: the launcher runs every tile whole (and touches no workspace)."""
    from view_fusion_amd import ops
    lib = ops._lib.load()
    d = wp.describe(c.kernel, c.S, c.Cin, c.Cout, c.H, c.H)
    t, r64, r32 = _refs(c, backward=False)
    y, _ = _abi_launch(lib, dev, c, t, ws_mode)
    _judge_all(_label(c, d) + f" | fallback ws {ws_mode}", ("y",), [y], r64, r32, (wp.TOL[c.kernel],))


# ------------------------------------------------------------------------------------------------ (d) GroupNorm in the fix-up
@pytest.mark.parametrize("S,Cin,Cout,H", wp.gn_cases(), ids=lambda v: str(v))
def test_fixup_groupnorm_per_plan_class(dev, S, Cin, Cout, H):
    from view_fusion_amd import ops
    lib = ops._lib.load()
    d = wp.describe("nested", S, Cin, Cout, H, H)
    assert lib.vf_wino_conv_gn_fusable(S, Cin, Cout, H, H, 0, 32) == 1 and d["nfull"] == 0 and d["split"] > 1
    assert lib.vf_wino_conv_ws_floats(S, Cin, Cout, H, H) == d["parts"] * wp.PART_FLOATS["nested"]
    conv, gn, x, vb, res, r64, r32 = cr.conv_gn_case(S, Cin, Cout, H, 1)
    conv, gn = conv.to(dev), gn.to(dev)
    ops.st.FORCE_WINOGRAD = True
    ops.st.KERNEL_LOG = []
    try:
        with torch.no_grad():
            y, a = ops.conv2d_gn(x.to(dev), conv, gn, 32, True, view_bias=vb.to(dev), residual=res.to(dev), want_y=True)
        torch.cuda.synchronize()
        log = [e[5] for e in ops.st.KERNEL_LOG if e[5] != "vf_wino_pack_weights"]
    finally:
        ops.st.KERNEL_LOG = None
        ops.st.FORCE_WINOGRAD = False
    assert log == ["vf_wino_conv_fwd_gn"], log
    label = f"nested {H}x{H} same S={S} {Cin}->{Cout} | T {d['T']} split {d['split']} per {d['per']} last {d['last']} | fix-up GroupNorm"
    _judge_all(label, ("y", "gn(y)"), [y, a], r64, r32, (cr.TOL["conv_gn"],) * 2)
