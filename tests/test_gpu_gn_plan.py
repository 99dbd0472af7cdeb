"""Every reachable launch plan of the GroupNorm(+Swish) forward / backward and the row / column sums of csrc/norm.hip on a
real MI355X, against float64.

The cases come from tests/gn_plan_ref.py:cases() -- every gn_fwd_kernel<NV, NT> instantiation on its threshold, at its
smallest n4, with a partly filled last slot and (NV > 1) a wholly empty one, at every map that reaches it, plain and on a
concatenated input whose boundary falls on a group edge, inside a group, inside the first and the last group and off a
multiple of four; the general kernels reached from a power-of-two map, from any other map and from HW < 4; all ten
gn_bwd_fused_kernel instantiations at threshold and smallest group on every map that reaches them, plain and concatenated;
the two-kernel backward on its maps, with 1, 2 and more chunks, S C % 4 = 0 .. 3 and a ragged add_inplace tail.
tests/test_gn_plan_host.py checks on the CPU that the restatement equals the library on the whole domain, that the list
holds every class the SMALL / TINY layers reach, and that the rule below rejects seven wrong models of the kernels.

(a) parity per class through the C ABI (vf_gn_cat_fwd, then vf_gn_cat_bwd fed with the forward kernel's own mean / rstd, as
ops does), the plan queried first (vf_gn_plan) and asserted equal to the restatement; every addend state, dx_rowsum requested
and NULL, both Swish values on the fused routes; (b) every output NaN-filled with a NaN guard behind it: exactly the
plan's floats written, a second run bit-identical; (c) a concatenated input bit-identical to the plain entry on the
materialised concatenation; (d) refusals write nothing; (e) through ops; (f) vf_rowsum / vf_bias_grad / vf_colsum /
vf_colsum_multi on the edges of their eight-slot loops.

The rule (cond_ref.judge): err = max|a - r64| / max|r64| <= max(4 e, tol), tol = cond_ref.TOL["gn_fwd"] = 1e-5 for y,
mean, rstd and TOL["gn_bwd"] = 2e-5 for dx, dgamma, dbeta (the partials summed over the views) and the sums of (f); r64 the
float64 restatement, e = stock fp32 CPU torch's error on the same inputs; any non-finite value fails.  dx_rowsum keeps
test_group_norm_backward_rowsum's bound: 2e-6 x the largest per-row sum of |dx|, against the float64 row sums of the
float64 dx without addends.  Measured values: profiles/gn_plan.md."""
import ctypes

import pytest
import torch

import cond_ref as cr
import gn_plan_ref as gp

pytestmark = pytest.mark.gpu

GUARD = 1024
NAN = float("nan")
INVALID = 1                      # hipErrorInvalidValue


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from view_fusion_amd import ops
    return ops._lib.load()


def _query(lib, C, HW, groups, cat, C1, a1, a2, dx2):
    out = (ctypes.c_int * 12)()
    assert lib.vf_gn_plan(C, HW, groups, int(cat), C1, int(a1), int(a2), int(dx2), ctypes.cast(out, ctypes.c_void_p)) == 0
    return list(out)


def _guarded(dev, *shape):
    """A NaN-filled tensor of `shape` with GUARD NaN floats behind it -> (view, whole buffer)."""
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + GUARD,), NAN, device=dev)
    return buf[:n].view(*shape), buf


def _written(buf, what):
    """Everything in front of the guard finite, the guard untouched."""
    assert bool(torch.isnan(buf[-GUARD:]).all()), f"written past {what}"
    assert bool(torch.isfinite(buf[:-GUARD]).all()), f"{what} not fully written"


def _untouched(buf, what):
    assert bool(torch.isnan(buf).all()), f"{what} written"


class _Run:
    """One case's device tensors and its calls through the C ABI; cat: split x (and dx, and the addend) at C1."""

    def __init__(self, lib, dev, c, t, cat):
        self.lib, self.dev, self.c, self.cat = lib, dev, c, cat
        self.t = {k: v.to(dev).contiguous() for k, v in t.items()}
        x = self.t["x"]
        self.x1, self.x2 = (x[:, :c.C1].contiguous(), x[:, c.C1:].contiguous()) if cat else (x, None)
        self.C1 = c.C1 if cat else c.C

    def fwd(self, silu, S=None):
        from view_fusion_amd.ops.core import _ptr, _stream
        c = self.c
        y, by = _guarded(self.dev, c.S, c.C, c.H, c.W)
        mean, bm = _guarded(self.dev, c.S * c.groups)
        rstd, br = _guarded(self.dev, c.S * c.groups)
        rc = self.lib.vf_gn_cat_fwd(_ptr(self.x1), _ptr(self.x2), self.C1, _ptr(self.t["gamma"]), _ptr(self.t["beta"]), _ptr(y),
                                    _ptr(mean), _ptr(rstd), c.S if S is None else S, c.C, c.H * c.W, c.groups, 1e-5, silu, _stream())
        torch.cuda.synchronize()
        return rc, dict(y=y, mean=mean.view(c.S, c.groups), rstd=rstd.view(c.S, c.groups)), (by, bm, br)

    def bwd(self, silu, state, mean, rstd, want_rowsum, S=None):
        from view_fusion_amd.ops.core import _ptr, _stream
        c, t = self.c, self.t
        if self.cat:
            dx1, b1 = _guarded(self.dev, c.S, c.C1, c.H, c.W)
            dx2, b2 = _guarded(self.dev, c.S, c.C - c.C1, c.H, c.W)
            dxb = [b1, b2]
            a1 = t["a1"][:, :c.C1].contiguous() if state != "none" else None
            a2 = t["a1"][:, c.C1:].contiguous() if state != "none" else None
        else:
            dx1, b1 = _guarded(self.dev, c.S, c.C, c.H, c.W)
            dx2, dxb = None, [b1]
            a1 = t["a1"] if state != "none" else None
            a2 = t["a2"] if state == "both" else None
        dg, bg = _guarded(self.dev, c.S, c.C)
        db, bb = _guarded(self.dev, c.S, c.C)
        rs, brs = _guarded(self.dev, c.S, c.C)
        rc = self.lib.vf_gn_cat_bwd(_ptr(self.x1), _ptr(self.x2), self.C1, _ptr(t["gamma"]), _ptr(t["beta"]), _ptr(mean), _ptr(rstd),
                                    _ptr(t["dy"]), _ptr(a1), _ptr(a2), _ptr(dx1), _ptr(dx2), _ptr(dg), _ptr(db),
                                    _ptr(rs) if want_rowsum else None, c.S if S is None else S, c.C, c.H * c.W, c.groups, silu, _stream())
        torch.cuda.synchronize()
        dx = torch.cat([dx1, dx2], 1) if self.cat else dx1
        return rc, dict(dx=dx, dgamma_part=dg, dbeta_part=db, rowsum=rs), dict(dx=dxb, parts=[bg, bb], rowsum=brs)


def _label(c, d):
    f = f"{gp.FWD_NAMES[d['fwd']]}" + (f"<{d['fnv']},{d['fnt']}>" if d["fwd"] == gp.FWD_REG else "")
    b = gp.BWD_NAMES[d["bwd"]] + (f" ({d['bnv']}, {d['bnt']}, {d['seg']}) lds {d['lds']}" if d["seg"] else "") \
        + (f" chunks {d['chunks']} adds {d['adds']}" if d["bwd"] == gp.BWD_TWO else "")
    return f"{gp.case_id(c)} | {f} -> {b}"


def _report(label, rows):
    for n, err, e, bound, ok in rows:
        print(f"GNPLAN | {label} | {n} | e {e:.3e} | err {err:.3e} | bound {bound:.3e} | {'ok' if ok else 'FAIL'}")
    return [(r[0], r[1], r[3]) for r in rows if not r[4]]


def _check_bwd(c, d, out, bufs, want_rowsum):
    """(b): dx and exactly S C floats of each partial written, dx_rowsum iff the plan says so, every guard intact."""
    for b in bufs["dx"]:
        _written(b, "dx")
    for b in bufs["parts"]:
        _written(b, "a partial")
    if want_rowsum and d["rowsum"]:
        _written(bufs["rowsum"], "dx_rowsum")
    else:
        _untouched(bufs["rowsum"], "dx_rowsum (not in the plan, or not requested)")


def _rowsum_row(label, rs, r64):
    err, bound = float((rs.double().cpu() - r64["rowsum"]).abs().max()), 2e-6 * r64["rowabs"]
    print(f"GNPLAN | {label} | dx_rowsum | e - | err {err:.3e} | bound {bound:.3e} | {'ok' if err <= bound else 'FAIL'}")
    return [] if err <= bound else [("dx_rowsum", err, bound)]


def _run_case(lib, dev, c, cat, second=None):
    """Forward, then the backward in every addend state -> {(silu, state, want_rowsum): outputs}; asserts (a) and (b)."""
    HW = c.H * c.W
    t = gp.inputs(c)
    if cat:
        t = gp.cat_addend(t, c)
    R = _Run(lib, dev, c, t, cat)
    d0 = gp.plan(c, "none", cat)
    fused = d0["bwd"] in (gp.BWD_FUSED16, gp.BWD_FUSED64)
    results, bad = {}, []
    print()
    for silu in ((c.silu, 1 - c.silu) if fused else (c.silu,)):
        r64, r32 = gp.refs(c, t, silu)
        rc, f, fb = R.fwd(silu)
        assert rc == 0
        for b, what in zip(fb, ("y", "mean", "rstd")):
            _written(b, what)
        bad += _report(_label(c, d0) + f" | silu {silu}", gp.judge_all(f, r64, r32, ("y", "mean", "rstd")))
        results[silu, "fwd"] = f
        for state in (("none", "both") if cat else gp.ADDEND_STATES):
            d = gp.plan(c, state, cat)
            a1, a2 = state != "none", (state != "none") if cat else state == "both"
            assert _query(lib, c.C, HW, c.groups, cat, R.C1, a1, a2, cat) == gp.fields(d), (gp.case_id(c), state, d)
            if d["bwd"] == gp.REJECTED:
                assert cat and not fused
                rc, out, bufs = R.bwd(silu, state, f["mean"], f["rstd"], True)
                assert rc == INVALID
                for b in bufs["dx"] + bufs["parts"] + [bufs["rowsum"]]:
                    _untouched(b, "an output of a refused backward")
                continue
            a64, a32 = gp.with_addends(r64, t, state, torch.float64), gp.with_addends(r32, t, state, torch.float32)
            for want_rowsum in (True, False):
                rc, out, bufs = R.bwd(silu, state, f["mean"], f["rstd"], want_rowsum)
                assert rc == 0
                _check_bwd(c, d, out, bufs, want_rowsum)
                results[silu, state, want_rowsum] = out
                if not want_rowsum:                      # (the sums must not depend on whether dx_rowsum is written)
                    prev = results[silu, state, True]
                    assert all(torch.equal(out[k], prev[k]) for k in ("dx", "dgamma_part", "dbeta_part"))
                    continue
                got = dict(dx=out["dx"], dgamma=out["dgamma_part"].double().sum(0), dbeta=out["dbeta_part"].double().sum(0))
                label = _label(c, d) + f" | silu {silu} | addends {state}"
                bad += _report(label, gp.judge_all(got, a64, a32, ("dx", "dgamma", "dbeta")))
                if d["rowsum"]:
                    bad += _rowsum_row(label, out["rowsum"], r64)
    assert not bad, bad
    return results


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        for n in a[k]:
            # (an untouched dx_rowsum is NaN in both)
            assert torch.equal(torch.nan_to_num(a[k][n], nan=-7.0), torch.nan_to_num(b[k][n], nan=-7.0)), (k, n)


# ------------------------------------------------------------------------------------------------ (a) (b) (c) per plan class
@pytest.mark.parametrize("c", gp.cases(), ids=gp.case_id)
def test_gn_plan_class_vs_fp64(dev, lib, c):
    """(a) + (b) on every case; (c) a concatenated input: bit-identical to the plain entry on the materialised concatenation
    (the addend concatenated the same way) wherever both run."""
    d = gp.plan(c)
    assert _query(lib, c.C, c.H * c.W, c.groups, bool(c.C1), c.C1 if c.C1 else c.C, 0, 0, bool(c.C1)) == gp.fields(d)
    res = _run_case(lib, dev, c, bool(c.C1))
    if c.C1:
        plain = _run_case(lib, dev, c, False)
        for k, v in res.items():
            if k[1] == "fwd":
                pk = k
            else:                                        # cat "both" = the plain entry with the one concatenated addend
                pk = (k[0], "addend" if k[1] == "both" else k[1], k[2])
            for n in v:
                assert torch.equal(torch.nan_to_num(v[n], nan=-7.0), torch.nan_to_num(plain[pk][n], nan=-7.0)), \
                    (gp.case_id(c), k, n, "cat differs from plain")


@pytest.mark.parametrize("c", gp.hygiene_cases(), ids=gp.case_id)
def test_gn_second_run_is_bit_identical(dev, lib, c):
    """(b): the whole sequence again on fresh NaN-filled buffers: every output bit-identical."""
    _same(_run_case(lib, dev, c, bool(c.C1)), _run_case(lib, dev, c, bool(c.C1)))


# ------------------------------------------------------------------------------------------------ (d) refusals
@pytest.mark.parametrize("args,which,why", gp.REJECTIONS, ids=lambda v: v.replace(" ", "-") if isinstance(v, str) and len(v) > 4 else None)
def test_refused_calls_write_nothing(dev, lib, args, which, why):
    from view_fusion_amd.ops.core import _ptr, _stream
    C, HW, groups, cat, C1, a1, a2, dx2 = args
    S = 2
    assert _query(lib, *args)[3] == gp.REJECTED and (_query(lib, *args)[0] == gp.REJECTED) == (which == "both")
    x = torch.rand(S, C, HW, device=dev)
    other = torch.rand(S, C, HW, device=dev)
    gamma, beta = torch.rand(C, device=dev), torch.rand(C, device=dev)
    ng = max(abs(groups), 1)
    y, by = _guarded(dev, S, C, HW)
    mean, bm = _guarded(dev, S * ng)
    rstd, br = _guarded(dev, S * ng)
    rc = lib.vf_gn_cat_fwd(_ptr(x), _ptr(other) if cat else None, C1, _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd), S, C,
                           HW, groups, 1e-5, 1, _stream())
    torch.cuda.synchronize()
    if which == "both":
        assert rc == INVALID
        for b in (by, bm, br):
            _untouched(b, "an output of a refused forward")
        mean, rstd = torch.zeros(S * ng, device=dev), torch.ones(S * ng, device=dev)
    else:
        assert rc == 0
    outs = [_guarded(dev, S, C, HW), _guarded(dev, S, C, HW), _guarded(dev, S, C), _guarded(dev, S, C), _guarded(dev, S, C)]
    (dx, _), (dx2t, _), (dg, _), (db, _), (rs, _) = outs
    rc = lib.vf_gn_cat_bwd(_ptr(x), _ptr(other) if cat else None, C1, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd), _ptr(other),
                           _ptr(other) if a1 else None, _ptr(other) if a2 else None, _ptr(dx), _ptr(dx2t) if dx2 else None, _ptr(dg),
                           _ptr(db), _ptr(rs), S, C, HW, groups, 1, _stream())
    torch.cuda.synchronize()
    assert rc == INVALID, why
    for _, b in outs:
        _untouched(b, "an output of a refused backward")


def test_no_views_is_no_work(dev, lib):
    """S = 0 returns 0 and writes nothing, on every backward route."""
    for c in (gp.mk(2, 4, 64), gp.mk(2, 4, 256), gp.mk(2, 3, 16), gp.mk(2, 3, 15), gp.mk(2, 4, 64, groups=3, C1=5)):
        R = _Run(lib, dev, c, gp.inputs(c), bool(c.C1))
        rc, f, fb = R.fwd(1, S=0)
        assert rc == 0
        for b in fb:
            _untouched(b, "a forward output at S = 0")
        rc, out, bufs = R.bwd(1, "both", torch.zeros(c.S * c.groups, device=dev), torch.ones(c.S * c.groups, device=dev), True, S=0)
        assert rc == 0
        for b in bufs["dx"] + bufs["parts"] + [bufs["rowsum"]]:
            _untouched(b, "a backward output at S = 0")


# ------------------------------------------------------------------------------------------------ (e) through ops
# (C, H, W): one shape per backward route -- 16-lane fused, 64-lane fused, two-kernel, general
OPS_SHAPES = ((64, 8, 8), (64, 16, 16), (64, 4, 4), (64, 6, 10))


def _logged(fn):
    from view_fusion_amd import ops
    ops.st.KERNEL_LOG = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, [e[5] for e in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None


@pytest.mark.parametrize("groups", [32, 8])
@pytest.mark.parametrize("shape", OPS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gn_through_ops(dev, lib, shape, groups):
    """ops.group_norm, group_norm_skip (with and without tap) and group_norm_cat_skip (both second consumers, one, none)
    with autograd on: the entries the kernel log names, ops.cat_fusable = the plan's answer, every gradient under the rule."""
    from view_fusion_amd import ops
    C, H, W = shape
    S, HW, C1 = 2, H * W, 23                             # (23: inside a group, off a multiple of four)
    c = gp.Case(S, C, H, W, groups, 0, 1, "")
    t = gp.inputs(c)
    r64, r32 = gp.refs(c, t, 1)
    d = gp.plan(c)
    dplan = gp.plan(c._replace(C1=C1), "both")
    assert bool(lib.vf_gn_bwd_emits_rowsum(C, HW, groups)) == bool(d["rowsum"]) == (dplan["bwd"] != gp.REJECTED)
    assert not ops.cat_fusable(C1, C, HW, groups), "a split off a multiple of 64 is materialised by the model"
    wide = gp.Case(S, 2 * C, H, W, groups, 64, 1, "")
    assert ops.cat_fusable(64, 2 * C, HW, groups) == (gp.plan(wide, "both")["bwd"] != gp.REJECTED)
    G = lambda k: t[k].to(dev)
    bad = []
    print()

    def leaves():
        return G("x").requires_grad_(True), G("gamma").requires_grad_(True), G("beta").requires_grad_(True)

    def check(label, y, x, ga, be, state, names, want):
        assert [n for n in names if n.startswith("vf_gn")] == want, (label, names)
        got = dict(y=y.detach(), dx=x.grad, dgamma=ga.grad, dbeta=be.grad)
        a64, a32 = gp.with_addends(r64, t, state, torch.float64), gp.with_addends(r32, t, state, torch.float32)
        return _report(f"{gp.case_id(c)} | {label} | {gp.BWD_NAMES[d['bwd']]}", gp.judge_all(got, a64, a32, ("y", "dx", "dgamma", "dbeta")))

    x, ga, be = leaves()
    y, names = _logged(lambda: (lambda y: (y.backward(G("dy")), y)[1])(ops.group_norm(x, ga, be, groups, True)))
    bad += check("ops.group_norm", y, x, ga, be, "none", names, ["vf_gn_fwd", "vf_gn_cat_bwd"])
    for tap in (False, True):
        x, ga, be = leaves()

        def step():
            out = ops.group_norm_skip(x, ga, be, groups, True, tap=tap)
            loss = (out[0] * G("dy")).sum() + (out[1] * G("a1")).sum() + ((out[2] * G("a2")).sum() if tap else 0)
            loss.backward()
            return out[0]
        y, names = _logged(step)
        bad += check(f"ops.group_norm_skip tap={tap}", y, x, ga, be, "both" if tap else "addend", names, ["vf_gn_fwd", "vf_gn_cat_bwd"])
    if dplan["bwd"] != gp.REJECTED:                      # the concatenated entry: where the plan takes it
        for use in ((1, 1), (1, 0), (0, 1), (0, 0)):
            _, ga, be = leaves()
            x1, x2 = G("x")[:, :C1].contiguous().requires_grad_(True), G("x")[:, C1:].contiguous().requires_grad_(True)

            def step():
                y, t1, t2 = ops.group_norm_cat_skip(x1, x2, ga, be, groups, True)
                loss = (y * G("dy")).sum()
                if use[0]:
                    loss = loss + (t1 * G("a1")[:, :C1]).sum()
                if use[1]:
                    loss = loss + (t2 * G("a1")[:, C1:]).sum()
                loss.backward()
                return y
            y, names = _logged(step)
            assert [n for n in names if n.startswith("vf_gn")] == ["vf_gn_cat_fwd", "vf_gn_cat_bwd"], names
            add = torch.zeros_like(t["a1"])
            if use[0]:
                add[:, :C1] = t["a1"][:, :C1]
            if use[1]:
                add[:, C1:] = t["a1"][:, C1:]
            tt = dict(t, a1=add)
            got = dict(y=y.detach(), dx=torch.cat([x1.grad, x2.grad], 1), dgamma=ga.grad, dbeta=be.grad)
            a64, a32 = gp.with_addends(r64, tt, "addend", torch.float64), gp.with_addends(r32, tt, "addend", torch.float32)
            bad += _report(f"{gp.case_id(c)} | ops.group_norm_cat_skip d1, d2 = {use} | {gp.BWD_NAMES[dplan['bwd']]}",
                           gp.judge_all(got, a64, a32, ("y", "dx", "dgamma", "dbeta")))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ (f) the row and column sums
SUM_TOL = cr.TOL["gn_bwd"]
S_EDGES = (1, 3, 4, 5, 31, 32, 33, 65)


def _draw(*shape, seed):
    return (cr._u(shape, seed) + 0.25).float()


def _sum_row(label, got, x, dims, bad):
    err, e, bound, ok = cr.judge(got, x.double().sum(dims), x.sum(dims), SUM_TOL)
    print(f"GNPLAN | {label} | sum | e {e:.3e} | err {err:.3e} | bound {bound:.3e} | {'ok' if ok else 'FAIL'}")
    if not ok:
        bad.append((label, err, bound))


def test_rowsum_on_the_edges_of_the_eight_slot_tail(dev, lib):
    """vf_rowsum: one wave per row, four rows per workgroup; lane_sum_f4's main loop takes 512 float4 a round, its tail the
    rest in eight clamped slots -- len / 4 either side of 64, of 448 (the tail's last slot), of 512 and past 1024."""
    from view_fusion_amd.ops.core import _ptr, _stream
    bad = []
    print()
    for n4 in (1, 63, 64, 65, 448, 449, 511, 512, 513, 1025):
        for rows in (1, 3, 4, 5):
            x = _draw(rows, 4 * n4, seed=n4 + rows)
            out, buf = _guarded(dev, rows)
            assert lib.vf_rowsum(_ptr(x.to(dev)), _ptr(out), rows, 4 * n4, _stream()) == 0
            torch.cuda.synchronize()
            _written(buf, "the row sums")
            _sum_row(f"vf_rowsum len/4 {n4} rows {rows}", out, x, 1, bad)
    assert not bad, bad


def test_bias_grad_on_the_edges_of_both_branches(dev, lib):
    """vf_bias_grad: HW / 4 either side of the short-row branch (<= 64: eight views in flight per wave, S in steps of 32)
    and in the long-row one, S either side of 4 and 32 and two rounds; db or dvb NULL."""
    from view_fusion_amd.ops.core import _ptr, _stream
    bad, C = [], 3
    print()
    for n4 in (1, 63, 64, 65, 513):
        for S in S_EDGES:
            dy = _draw(S, C, 4 * n4, seed=n4 + S)
            g = dy.to(dev)
            for use_db, use_dvb in ((1, 1), (0, 1), (1, 0)):
                db, bdb = _guarded(dev, C)
                dvb, bdvb = _guarded(dev, S, C)
                assert lib.vf_bias_grad(_ptr(g), _ptr(db) if use_db else None, _ptr(dvb) if use_dvb else None, S, C, 4 * n4, _stream()) == 0
                torch.cuda.synchronize()
                for used, b, what, dims, out in ((use_db, bdb, "db", (0, 2), db), (use_dvb, bdvb, "dvb", 2, dvb)):
                    if used:
                        _written(b, what)
                        _sum_row(f"vf_bias_grad HW/4 {n4} S {S} {what}" + ("" if use_db and use_dvb else " alone"), out, dy, dims, bad)
                    else:
                        _untouched(b, what + " (NULL passed)")
    assert not bad, bad


def test_colsum_on_the_edges_of_the_row_stride(dev, lib):
    """vf_colsum: 64 columns x 4 row groups per workgroup, eight rows in flight per thread (S in steps of 32)."""
    from view_fusion_amd.ops.core import _ptr, _stream
    bad = []
    print()
    for S in S_EDGES:
        for C in (1, 63, 64, 65, 130):
            for batch in (1, 2):
                p = _draw(batch, S, C, seed=S + C + batch)
                out, buf = _guarded(dev, batch, C)
                assert lib.vf_colsum(_ptr(p.to(dev)), _ptr(out), batch, S, C, _stream()) == 0
                torch.cuda.synchronize()
                _written(buf, "the column sums")
                _sum_row(f"vf_colsum S {S} C {C} batch {batch}", out, p, 1, bad)
    assert not bad, bad


def test_colsum_multi_equals_the_single_launches(dev, lib):
    """vf_colsum_multi over a table with a one-block row between two multi-block rows (the first_block search): under the
    rule, and bit-identical to one vf_colsum per row."""
    from view_fusion_amd.ops.core import _ptr, _stream
    table = ((5, 130, 2), (33, 1, 1), (65, 65, 2), (1, 64, 1), (4, 200, 1), (31, 63, 3))      # (S, C, batch)
    parts = [_draw(b, S, C, seed=90 + i) for i, (S, C, b) in enumerate(table)]
    dparts = [p.to(dev) for p in parts]
    outs = [_guarded(dev, b, C) for S, C, b in table]
    rows, first = [], 0
    for (S, C, b), p, (o, _) in zip(table, dparts, outs):
        rows.append([p.data_ptr(), o.data_ptr(), S, C, b, first])
        first += (C + 63) // 64 * b
    assert [r[5] for r in rows] == [0, 6, 7, 11, 12, 16] and first == 19
    desc = torch.tensor(rows, dtype=torch.int64, device=dev)
    assert lib.vf_colsum_multi(_ptr(desc), len(rows), first, _stream()) == 0
    torch.cuda.synchronize()
    bad = []
    print()
    for (S, C, b), p, dp, (o, buf) in zip(table, parts, dparts, outs):
        _written(buf, "a row's column sums")
        _sum_row(f"vf_colsum_multi S {S} C {C} batch {b}", o, p, 1, bad)
        single, sb = _guarded(dev, b, C)
        assert lib.vf_colsum(_ptr(dp), _ptr(single), b, S, C, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(single, o), (S, C, b)
    assert not bad, bad
