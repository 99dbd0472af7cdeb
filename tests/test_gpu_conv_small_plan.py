"""Every launch plan of the sampler's one-launch convolutions (csrc/conv_small.hip: conv1_small_kernel<CAT>,
conv3_small_kernel<LOGTC, RS, PACKED>, conv3_small_pack_kernel) on a real MI355X, against float64.

The cases come from tests/conv_small_plan_ref.py:cases() -- the cheapest representative of every class its docstring
lists: all fourteen instantiations, the rounds (1, 2, >= 3, each with a full or half last round) under each form of the
main loop, the per-wave shares of the 1x1 and folded K loops (whole, partly filled, empty waves, the K - 4 clamp, a second
trip), Cout % tile, a concatenation boundary on and off a multiple of four, every epilogue operand present and absent,
GroupNorm on load (one channel per group, several, a group across two waves, both limits), output statistics, the
Upsample conv.  tests/test_conv_small_plan_host.py checks on the CPU that the restatement equals the library, that the
list holds every class the SMALL / TINY sampler layers reach, and that the rule below rejects seven wrong models.

(a) parity per case through its own C-ABI entry (vf_conv_small, vf_conv_small_res or vf_conv_small_gn), the plan queried
first (vf_conv_small_plan) and asserted equal to the restatement; (b) y NaN-filled between two NaN guard bands and
out_stats zero between two sentinel bands: exactly S Cout H W outputs and S Cout 2 sums written, a second launch
bit-identical; (c) the packed launch bit-identical to the unpacked one, vf_conv_small_res bit-identical to
vf_conv_small_gn; (d) a view alone (RS = 1) bit-identical to the same view in a batch past the RS = 2 threshold; (e) the
integer sums against float64 sums of the kernel's own y; (f) refusals and S = 0 write nothing; (g) through ops at the
natural thresholds, packed and not.

The rule (cond_ref.judge): err = max|a - r64| / max|r64| <= max(4 e, tol), tol = cond_ref.TOL["small_h"] = 2e-6 for a conv
output and TOL["small_y"] = 5e-6 behind GroupNorm on load; r64 the float64 convolution, e = stock fp32 CPU torch's error on
the same inputs; any non-finite value fails.  Measured values: profiles/conv_small_plan.md."""
import ctypes

import pytest
import torch

import cond_ref as cr
import conv_small_plan_ref as sp

pytestmark = pytest.mark.gpu

GUARD = 1024
NAN = float("nan")
SENTINEL = 0x5A5A5A5A5A5A5A5A
_MODE_NAMES = {0: "same", 1: "down2", 2: "up2"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from view_fusion_amd import ops
    return ops._lib.load()


def _query(lib, **args):
    out = (ctypes.c_int * 16)()
    assert lib.vf_conv_small_plan(*(int(args[k]) for k in sp.ARGS), ctypes.cast(out, ctypes.c_void_p)) == 0
    return list(out)


def _guarded_y(dev, n):
    buf = torch.full((n + 2 * GUARD,), NAN, device=dev)
    return buf[GUARD:GUARD + n], buf


def _guarded_stats(dev, n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    buf[GUARD:GUARD + n] = 0
    return buf[GUARD:GUARD + n], buf


def _y_written(buf, what):
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), f"written outside {what}"
    assert bool(torch.isfinite(buf[GUARD:-GUARD]).all()), f"{what} not fully written"


def _stats_written(buf, n):
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), "written outside out_stats"
    assert bool((buf[GUARD:-GUARD].view(-1, 2)[:, 1] > 0).all()), "a sum of squares not written"


class _Run:
    """One case's device tensors and its launches through the C ABI."""

    def __init__(self, lib, dev, c, t):
        self.lib, self.dev, self.c = lib, dev, c
        g = lambda v: None if v is None else v.to(dev).contiguous()
        self.t = {k: g(v) for k, v in t.items()}
        x = self.t["x"]
        self.x1, self.x2 = (x[:, :c.C1].contiguous(), x[:, c.C1:].contiguous()) if c.C1 else (x, None)
        rx = self.t["rx"]
        self.rx1, self.rx2 = (rx[:, :c.rC1].contiguous(), rx[:, c.rC1:].contiguous()) if c.rC1 else (rx, None)
        self.ist = sp.in_stats(t["x"]).to(dev).contiguous() if c.groups else None
        self.wp = None

    def packed(self):
        from view_fusion_amd.ops.core import _ptr, _stream
        if self.wp is None:
            c = self.c
            n = self.lib.vf_conv_small_pack_floats(c.Cout, c.Cin)
            wp, buf = _guarded_y(self.dev, n)
            assert self.lib.vf_conv_small_pack(_ptr(self.t["w"]), _ptr(wp), c.Cout, c.Cin, _stream()) == 0
            torch.cuda.synchronize()
            _y_written(buf, "the packed weights")
            self.wp = wp
        return self.wp

    def launch(self, entry=None, packed=None, views=None):
        """-> (rc, y, out_stats | None, (y buffer, stats buffer | None)); views: a slice of the batch run as its own call."""
        from view_fusion_amd.ops.core import _ptr, _stream
        c, t = self.c, self.t
        entry = sp.entry(c) if entry is None else entry
        packed = c.packed if packed is None else packed
        v = slice(0, c.S) if views is None else views
        S = len(range(*v.indices(c.S)))
        cut = lambda a: None if a is None else a[v].contiguous()
        x1, x2, vb, res, rx1, rx2, ist = (cut(a) for a in (self.x1, self.x2, t["vbias"], t["residual"], self.rx1, self.rx2, self.ist))
        y, ybuf = _guarded_y(self.dev, S * c.Cout * c.H * c.H)
        ost, obuf = _guarded_stats(self.dev, S * c.Cout * 2) if c.ostats else (None, None)
        P = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr())
        if entry == "vf_conv_small":
            assert not (c.groups or c.ostats or c.rC or packed)
            rc = self.lib.vf_conv_small(P(x1), P(x2), c.C1, P(t["w"]), P(t["bias"]), P(vb), P(res), P(y), S, c.Cin, c.Cout, c.H,
                                        c.H, c.KS, c.mode, _stream())
        elif entry == "vf_conv_small_res":
            assert c.rC and not (c.groups or c.ostats or packed or c.residual)
            rc = self.lib.vf_conv_small_res(P(x1), P(t["w"]), P(t["bias"]), P(vb), P(y), S, c.Cin, c.Cout, c.H, c.H, P(rx1), P(rx2),
                                            c.rC1, c.rC, P(t["rw"]), P(t["rbias"]), _stream())
        else:
            rc = self.lib.vf_conv_small_gn(P(x1), P(x2), c.C1, P(t["w"]), P(t["bias"]), P(vb), P(res), P(y), S, c.Cin, c.Cout, c.H,
                                           c.H, c.KS, P(ist), P(t["gamma"]), P(t["beta"]), c.groups, cr.EPS, c.silu, P(ost),
                                           P(rx1), P(rx2), c.rC1, c.rC, P(t["rw"]), P(t["rbias"]),
                                           P(self.packed()) if packed else None, c.mode, _stream())
        torch.cuda.synchronize()
        return rc, y.view(S, c.Cout, c.H, c.H), (ost.view(S, c.Cout, 2) if ost is not None else None), (ybuf, obuf)


def _inst(d):
    if d["kernel"] == sp.K_3X3:
        return f"conv3_small_kernel<{d['logtc']},{d['rs']},{'true' if d['packed'] else 'false'}>"
    return f"conv1_small_kernel<{'true' if d['kernel'] == sp.K_CAT else 'false'}>"


def _stats_check(label, c, y, ost):
    """(e): the integer sums against float64 sums of the kernel's own fp32 y.  Every workgroup adds, per channel, the sum of
    its 16 pixels rounded once to the 2^-24 unit: at most half a unit each, (tiles per channel) 2^-25 in all; the float64
    sums themselves (the kernel's 16-term ones and the H W-term ones here) err by at most (terms) 2^-53 of sum |.|."""
    tiles = c.H * c.H // 16
    yd = y.double()
    bad = []
    for i, (name, v) in enumerate((("sum y", yd), ("sum y^2", yd * yd))):
        want = v.sum((2, 3))
        own = 2.0 * c.H * c.H * 2.0 ** -53 * float(v.abs().sum((2, 3)).max())
        off = float((ost[..., i].double() / 2.0 ** 24 - want).abs().max())
        bound = tiles * 2.0 ** -25 + own
        print(f"SMALLPLAN | {label} | {name} | off {off:.3e} | bound {bound:.3e} | ratio {off / bound:.3f} | {'ok' if off <= bound else 'FAIL'}")
        if off > bound:
            bad.append((name, off, bound))
    return bad


# ------------------------------------------------------------------------------------------------ (a) (b) (e) per class
@pytest.mark.parametrize("c", sp.cases(), ids=sp.case_id)
def test_conv_small_plan_class_vs_fp64(dev, lib, c):
    d = sp.plan(c)
    assert _query(lib, **sp.plan_args(c)) == sp.fields(d), (sp.case_id(c), d)
    t = sp.inputs(c)
    r64, r32 = sp.refs(c, t)
    R = _Run(lib, dev, c, t)
    rc, y, ost, (ybuf, obuf) = R.launch()
    assert rc == 0
    _y_written(ybuf, "y")
    if c.ostats:
        _stats_written(obuf, c.S * c.Cout * 2)
    rc, y2, ost2, _ = R.launch()
    assert rc == 0 and torch.equal(y, y2) and (ost is None or torch.equal(ost, ost2)), "a second launch differs"
    err, e, bound, ok = cr.judge(y, r64, r32, sp.tol(c))
    label = f"{sp.case_id(c)} | {sp.entry(c)} | {_inst(d)}"
    print(f"\nSMALLPLAN | {label} | y | e {e:.3e} | err {err:.3e} | bound {bound:.3e} | ratio {err / bound:.3f} | {'ok' if ok else 'FAIL'}")
    bad = [] if ok else [("y", err, bound)]
    if c.ostats:
        bad += _stats_check(label, c, y, ost)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ (c) equivalences
@pytest.mark.parametrize("c", sp.pairs_3x3(), ids=sp.case_id)
def test_packed_launch_equals_the_unpacked_one(dev, lib, c):
    """Both forms issue the same values to the same MFMA sequence: bit-identical y and sums, through the general entry."""
    assert sp.plan(c, wp=1)["packed"] == 1 and sp.plan(c, wp=0)["packed"] == 0
    R = _Run(lib, dev, c, sp.inputs(c))
    rc0, y0, o0, _ = R.launch(entry="vf_conv_small_gn", packed=0)
    rc1, y1, o1, (ybuf, _) = R.launch(entry="vf_conv_small_gn", packed=1)
    assert rc0 == 0 and rc1 == 0
    _y_written(ybuf, "y")
    assert torch.equal(y0, y1) and (o0 is None or torch.equal(o0, o1))


@pytest.mark.parametrize("c", [c for c in sp.fold_cases() if sp.entry(c) == "vf_conv_small_res"], ids=sp.case_id)
def test_res_entry_equals_the_general_entry(dev, lib, c):
    R = _Run(lib, dev, c, sp.inputs(c))
    rc0, y0, _, _ = R.launch(entry="vf_conv_small_res")
    rc1, y1, _, _ = R.launch(entry="vf_conv_small_gn")
    assert rc0 == 0 and rc1 == 0 and torch.equal(y0, y1)


def test_every_entry_and_instantiation_is_launched(lib):
    """What the parametrised tests above launch, from the plan rows the library itself reports."""
    seen, entries = set(), set()
    for c in sp.cases():
        r = _query(lib, **sp.plan_args(c))
        seen.add(tuple(r[1:5]))
        entries.add(sp.entry(c))
    want = {(sp.K_1X1, 0, 2, 0), (sp.K_CAT, 0, 2, 0)} | {(sp.K_3X3, l, rs, p) for l in (4, 3, 2) for rs in (1, 2) for p in (0, 1)}
    assert seen == want and entries == {"vf_conv_small", "vf_conv_small_res", "vf_conv_small_gn"}


# ------------------------------------------------------------------------------------------------ (d) batch invariance
@pytest.mark.parametrize("packed", [0, 1], ids=["unpacked", "packed"])
@pytest.mark.parametrize("H,S,mode", [(16, 16, 0), (8, 64, 2), (4, 64, 0)], ids=["16x16", "8x8-up", "4x4"])
def test_a_view_alone_equals_the_view_in_a_batch_across_the_rs_switch(dev, lib, H, S, mode, packed):
    """The batch takes 32-channel workgroups (RS = 2), a single view 16-channel ones (RS = 1): every output element is the
    same eight partial sums of the same MFMA sequence, added in the same order -- bit-identical, sums included."""
    Cout = 100 if H == 4 else 20
    c = sp.mk(S, 96, Cout, H, mode=mode, bias=1, vbias=1, residual=1, ostats=1, packed=packed)
    one = c._replace(S=1)
    assert sp.plan(c)["rs"] == 2 and sp.plan(one)["rs"] == 1
    t = sp.inputs(c)
    R = _Run(lib, dev, c, t)
    rc, y, ost, _ = R.launch()
    assert rc == 0
    err, e, bound, ok = cr.judge(y, *sp.refs(c, t), sp.tol(c))
    print(f"\nSMALLPLAN | {sp.case_id(c)} | batch | e {e:.3e} | err {err:.3e} | bound {bound:.3e} | ratio {err / bound:.3f}")
    assert ok, (err, bound)
    for s in (0, S // 2, S - 1):
        rc, ys, os_, (ybuf, obuf) = R.launch(views=slice(s, s + 1))
        assert rc == 0
        _y_written(ybuf, "y of one view")
        _stats_written(obuf, Cout * 2)
        same = torch.equal(ys[0], y[s]) and torch.equal(os_[0], ost[s])
        print(f"SMALLPLAN | {sp.case_id(c)} | view {s} alone vs in the batch | {'bit-identical' if same else 'DIFFERS'}")
        assert same, s


# ------------------------------------------------------------------------------------------------ (f) refusals
def _call_with_flags(lib, dev, a, pool, y, ost):
    """vf_conv_small_gn with the operand presence of plan_args `a`; every present operand points into `pool`."""
    from view_fusion_amd.ops.core import _stream
    P = lambda on: ctypes.c_void_p(pool.data_ptr()) if on else None
    return lib.vf_conv_small_gn(P(1), P(a["x2"]), a["C1"], P(1), P(1), P(1), P(a["residual"]), ctypes.c_void_p(y.data_ptr()), a["S"],
                                a["Cin"], a["Cout"], a["H"], a["W"], a["KS"], P(a["ist"]), P(a["affine"]), P(a["affine"]), a["groups"],
                                cr.EPS, 1, ctypes.c_void_p(ost.data_ptr()) if a["ost"] else None, P(a["rx"]), P(a["rx2"]), a["rC1"],
                                a["rC"], P(a["rw"]), P(1), P(a["wp"]), a["mode"], _stream())


@pytest.mark.parametrize("code,c,over", sp.REJECTIONS, ids=[f"{r[0]}-{sp.case_id(r[1])}" + "".join(f"-{k}{v}" for k, v in r[2].items()) for r in sp.REJECTIONS])
def test_refused_calls_write_nothing(dev, lib, code, c, over):
    a = dict(sp.plan_args(c, **over), ost=1)
    row = _query(lib, **a)
    assert row[0] == code and not any(row[1:]), (sp.REFUSALS[code], row)
    pool = torch.rand(1 << 20, device=dev)
    y, ybuf = _guarded_y(dev, max(c.S * max(c.Cout, 1) * c.H * c.H, 16))
    ost, obuf = _guarded_stats(dev, max(c.S * max(c.Cout, 1) * 2, 2))
    ost.fill_(SENTINEL)
    rc = _call_with_flags(lib, dev, a, pool, y, ost)
    torch.cuda.synchronize()
    assert rc == sp.INVALID, sp.REFUSALS[code]
    assert bool(torch.isnan(ybuf).all()) and bool((obuf == SENTINEL).all()), "a refused call wrote"


def test_entry_level_refusals_and_no_views(dev, lib):
    """vf_conv_small_res without rx, vf_conv_small_pack off its domain: refused, nothing written.  S = 0 (and below) through
    each of the three entries: 0, nothing written."""
    from view_fusion_amd.ops.core import _stream
    pool = torch.rand(1 << 16, device=dev)
    p = ctypes.c_void_p(pool.data_ptr())
    y, ybuf = _guarded_y(dev, 4096)
    ost, obuf = _guarded_stats(dev, 64)
    ost.fill_(SENTINEL)
    yp, op = ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(ost.data_ptr())
    assert lib.vf_conv_small_res(p, p, p, p, yp, 2, 32, 5, 4, 4, None, None, 8, 8, p, p, _stream()) == sp.INVALID
    assert lib.vf_conv_small_pack(p, yp, 5, 48, _stream()) == sp.INVALID
    assert lib.vf_conv_small_pack(p, yp, 0, 32, _stream()) == sp.INVALID
    for S in (0, -3):
        assert _query(lib, **dict(sp.plan_args(sp.mk(2, 32, 5, 4)), S=S))[:2] == [0, sp.K_NONE]
        assert lib.vf_conv_small(p, None, 0, p, p, p, p, yp, S, 32, 5, 4, 4, 3, 0, _stream()) == 0
        assert lib.vf_conv_small(p, p, 3, p, p, p, p, yp, S, 8, 5, 4, 4, 1, 0, _stream()) == 0
        assert lib.vf_conv_small_res(p, p, p, p, yp, S, 32, 5, 4, 4, p, p, 3, 8, p, p, _stream()) == 0
        assert lib.vf_conv_small_gn(p, None, 0, p, p, p, None, yp, S, 32, 5, 4, 4, 3, p, p, p, 8, cr.EPS, 1, op, None, None, 0, 0,
                                    None, None, None, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(ybuf).all()) and bool((obuf == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ (g) through ops
def _logged(fn):
    from view_fusion_amd import ops
    ops.st.KERNEL_LOG = []
    try:
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        return out, [e[5] for e in ops.st.KERNEL_LOG if e[5] != "vf_conv_small_pack"]
    finally:
        ops.st.KERNEL_LOG = None


def _layers(dev, c, t):
    conv = torch.nn.Conv2d(c.Cin, c.Cout, c.KS, padding=c.KS // 2, bias=bool(c.bias))
    res = torch.nn.Conv2d(c.rC, c.Cout, 1) if c.rC else None
    with torch.no_grad():
        conv.weight.copy_(t["w"])
        if c.bias:
            conv.bias.copy_(t["bias"])
        if res is not None:
            res.weight.copy_(t["rw"])
            res.bias.copy_(t["rbias"])
    return conv.to(dev), (res.to(dev) if res is not None else None)


@torch.no_grad()                                         # (the policy only takes these routes with autograd off)
def _ops_sweep(dev, S, pack):
    """Every convolution call of the SMALL / TINY no-grad forward at S views under the natural thresholds: the kernel log
    equals the restated policy; where the one-launch kernel runs, y passes the fp64 rule at its bare tolerance (e = 0)."""
    from view_fusion_amd import ops
    nat = dict(wgs1=ops.st.SMALL_CONV_MAX_WGS[0], wgs3=ops.st.SMALL_CONV_MAX_WGS[1], cin3=ops.st.SMALL_CONV_MAX_CIN3, s3=ops.st.SMALL_CONV_MAX_S3)
    assert nat == sp.NATURAL and ops.st.SMALL_PACK == pack
    bad, ran = [], set()
    G = lambda v: None if v is None else v.to(dev)
    print()
    for L in sp.model_layers():
        c = sp.layer_case(L, S, pack)
        if c.rC:
            small = sp.can_fold(S, c.Cout, c.H, c.H, c.rC)
            if not small:                                # (the model only offers the fold where can_fold_residual says so)
                assert not ops.can_fold_residual(S, c.Cout, c.H, c.H, torch.nn.Conv2d(c.rC, c.Cout, 1))
                continue
        else:
            small = sp.use_small(S, c.Cin, c.Cout, c.H, c.H, c.KS, c.mode)
        Hs = c.H * 2 if c.mode == 1 else (c.H // 2 if c.mode == 2 else c.H)
        if c.C1 and not small and not ops.cat_fusable(c.C1, c.Cin, c.H * c.H, 32):
            continue                                     # (the model materialises this concatenation)
        if small:
            t = sp.inputs(c)
        else:                                            # (only the route is checked: device-drawn operands)
            t = dict(x=torch.rand(S, c.Cin, Hs, Hs, device=dev), w=torch.rand(c.Cout, c.Cin, c.KS, c.KS) / (c.Cin * 9),
                     bias=torch.rand(c.Cout) if c.bias else None, vbias=torch.rand(S, c.Cout) if c.vbias else None,
                     residual=torch.rand(S, c.Cout, c.H, c.H, device=dev) if c.residual else None, rx=None, rw=None, rbias=None)
        conv, res = _layers(dev, c, t)
        x = G(t["x"])
        if c.C1:
            x1, x2 = x[:, :c.C1].contiguous(), x[:, c.C1:].contiguous()
            call = lambda: ops.conv1x1_cat(x1, x2, conv)
        elif c.rC:
            rx = G(t["rx"])
            fold = (res, rx[:, :c.rC1].contiguous(), rx[:, c.rC1:].contiguous()) if c.rC1 else (res, rx, None)
            assert ops.can_fold_residual(S, c.Cout, c.H, c.H, res)
            call = lambda: ops.conv2d(G(t["x"]), conv, view_bias=G(t["vbias"]), res_fold=fold)
        else:
            call = lambda: ops.conv2d(x, conv, view_bias=G(t["vbias"]), residual=G(t["residual"]), mode=_MODE_NAMES[c.mode])
        y, names = _logged(call)
        convs = [n for n in names if n.startswith("vf_conv_small")]
        if not small:
            assert not convs, (sp.case_id(c), names)
            continue
        want = "vf_conv_small" if c.KS == 1 else ("vf_conv_small_gn" if pack else ("vf_conv_small_res" if c.rC else "vf_conv_small"))
        assert names == [want], (sp.case_id(c), names)
        ran.add(want)
        r64 = sp.reference(c, t, torch.float64)
        err, _, bound, ok = cr.judge(y, r64, r64, sp.tol(c))
        print(f"SMALLPLAN | ops S {S} pack {int(pack)} | {sp.case_id(c)} | {want} | err {err:.3e} | bound {bound:.3e} | ratio {err / bound:.3f} | {'ok' if ok else 'FAIL'}")
        if not ok:
            bad.append((sp.case_id(c), err, bound))
        # a block's first conv: conv2d_gn = this launch + the GroupNorm launch (unless the Winograd fix-up takes the pair)
        if c.KS == 3 and c.vbias and not c.rC and ops.wino_kind(S, c.Cin, c.Cout, c.H, c.H, 3, c.mode, False) != 1:
            gn = torch.nn.GroupNorm(32, c.Cout).to(dev)
            with torch.no_grad():
                gn.weight.copy_(1 + 0.2 * cr._u((c.Cout,), 5)); gn.bias.copy_(0.2 * cr._u((c.Cout,), 6))
            (y2, a), names = _logged(lambda: ops.conv2d_gn(x, conv, gn, 32, True, view_bias=G(t["vbias"])))
            assert names[0] == want and len(names) == 2 and names[1].startswith("vf_gn"), names
            assert torch.equal(y2, y)
            a64 = cr.gn_forward_f64(r64, gn.weight.detach().cpu(), gn.bias.detach().cpu(), True)
            err, _, bound, ok = cr.judge(a, a64, a64, cr.TOL["gn_fwd"])
            print(f"SMALLPLAN | ops S {S} pack {int(pack)} | {sp.case_id(c)} | conv2d_gn a | err {err:.3e} | bound {bound:.3e} | {'ok' if ok else 'FAIL'}")
            if not ok:
                bad.append((sp.case_id(c) + " gn", err, bound))
    assert not bad, bad
    return ran


@pytest.mark.parametrize("S", [1, 2, 6, 12])
def test_routes_through_ops_at_the_natural_thresholds(dev, lib, S):
    ran = _ops_sweep(dev, S, True)
    assert "vf_conv_small" in ran and (S > 1 or "vf_conv_small_gn" in ran), ran


def test_routes_through_ops_without_the_packed_copy(dev, lib):
    """ops.st.SMALL_PACK off: the unpacked 3x3 kernels through vf_conv_small and vf_conv_small_res."""
    from view_fusion_amd import ops
    saved = ops.st.SMALL_PACK
    ops.st.SMALL_PACK = False
    try:
        ran = _ops_sweep(dev, 1, False)
    finally:
        ops.st.SMALL_PACK = saved
    assert ran == {"vf_conv_small", "vf_conv_small_res"}, ran


def test_tiny_unet_is_bit_identical_without_the_packed_copy(dev, lib):
    from conftest import TINY
    from view_fusion_amd import UNet, ops
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    net = net.to(dev).eval()
    x = cr._u((1, 6, 16, 16), 3).float().to(dev)
    angle, time = torch.tensor([[0.7]], device=dev), torch.tensor([[0.4]], device=dev)
    _logged(lambda: net(x, angle, time))                 # (the packed copies of every format are made once, here)
    y0, n0 = _logged(lambda: net(x, angle, time))
    saved = ops.st.SMALL_PACK
    ops.st.SMALL_PACK = False
    try:
        y1, n1 = _logged(lambda: net(x, angle, time))
    finally:
        ops.st.SMALL_PACK = saved
    assert "vf_conv_small_gn" in n0 and "vf_conv_small_gn" not in n1 and "vf_conv_small_res" in n1, (n0, n1)
    assert [n for n in n0 if not n.startswith("vf_conv_small")] == [n for n in n1 if not n.startswith("vf_conv_small")]
    assert bool(torch.isfinite(y0).all()) and torch.equal(y0, y1)
