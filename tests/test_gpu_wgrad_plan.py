"""Every reachable slab plan of the four weight-gradient launchers on a real MI355X, against float64.

The cases come from tests/wgrad_plan_ref.py:cases() -- per family (direct 3x3, 1x1, F(4x4), the general kernel) the
cheapest representative of every plan class (slices of 1 / 2 / 3 or more units, a short last slice, a half-empty 8x8
tile, a partly filled last step, the four 1x1 tile variants with padded channels and a concatenated input, with and
without the bias sums), of every class of the slab sum (1, 2-4, 5-32, 33-63, whole and ragged trips of 32 slabs), and a
few hand-written layers.  tests/test_wgrad_plan_host.py checks on the CPU that the list holds every class the SMALL /
TINY layers reach and that the rule below rejects a slab decomposition with a dropped unit, shifted ranges, a skipped
slab, an image read twice or the padded rows folded in.

(a) parity per plan class through the C ABI, the plan the launch took read back from the row its _main twin writes;
(b) NaN-filled outputs and workspace with a NaN guard behind it, twice, bit-identical, nothing written past z slabs;
(c) a workspace of one slab / half the slabs / one float short; (d) one deferred table with rows of all four planners;
(e) through ops.conv2d / ops.conv1x1_cat at the default policy, deferred and not.

The rule (cond_ref.judge): err = max|a - r64| / max|r64| <= max(4 e, tol), r64 = F.conv2d's weight gradient in float64
on the CPU, e = stock fp32 CPU torch's error on the same inputs, tol = 1e-4 for dW, 2e-5 for db / db2; any non-finite
value fails.  Measured values: profiles/wgrad_plan.md."""
import ctypes
import struct

import pytest
import torch

import cond_ref as cr
import wgrad_plan_ref as wp

pytestmark = pytest.mark.gpu

wp.check_env()

GUARD = 4096
INVALID_VALUE = 1           # hipErrorInvalidValue
NAN = float("nan")
_REFS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _refs(c):
    """(inputs, r64, r32) of a case; the references (a few kilobytes) are computed once and left unchanged."""
    key = (c.S, c.Cin, c.Cout, c.H, c.W, c.KS, c.mode)
    t = wp.inputs(c)
    if key not in _REFS:
        full = c._replace(db=2)
        _REFS[key] = (wp.wgrad_ref(t, full, torch.float64), wp.wgrad_ref(t, full, torch.float32))
    r64, r32 = _REFS[key]
    return t, r64[:1 + c.db], r32[:1 + c.db]


def _label(c, d):
    return (f"{wp.case_id(c)} | {d['variant']} units {d['units']} z {d['z']} per {d['per']} last {d['last']}"
            f"{' half' if d['half'] else ''}{' partial' if d['partial_step'] else ''}")


def _judge_all(label, c, got, r64, r32):
    rows = [(n, *cr.judge(a, b, f, tol)) for n, a, b, f, tol in zip(wp.NAMES, got, r64, r32, wp.tols(c))]
    print()
    for n, err, e, bound, ok in rows:
        print(f"WGRAD | {label} | {n} | e {e:.3e} | err {err:.3e} | bound {bound:.3e} | {'ok' if ok else 'FAIL'}")
    assert all(r[4] for r in rows), [(r[0], r[1], r[3]) for r in rows if not r[4]]


class _Launch:
    """One case's device tensors and its calls through the C ABI."""

    def __init__(self, lib, dev, c, t):
        self.lib, self.dev, self.c = lib, dev, c
        x, self.gy = t["x"].to(dev), t["gy"].to(dev).contiguous()
        self.x1, self.x2 = (x[:, :c.C1].contiguous(), x[:, c.C1:].contiguous()) if c.C1 else (x.contiguous(), None)

    def outputs(self):
        """NaN-filled dW, db, db2 (None where the case has none)."""
        c = self.c
        return [torch.full((c.Cout, c.Cin, c.KS, c.KS), NAN, device=self.dev)] + \
               [torch.full((c.Cout,), NAN, device=self.dev) if c.db > k else None for k in (0, 1)]

    def workspace(self, floats):
        return torch.full((floats + GUARD,), NAN, device=self.dev)

    def run(self, out, ws, ws_floats, main=False):
        """-> (return code, row | None).  main: the _main twin (no slab sum), whose row is parsed."""
        from view_fusion_amd.ops.core import _ptr, _stream
        c = self.c
        dw, db, db2 = out
        dims = (c.S, c.Cin, c.Cout, c.H, c.W)
        if c.family == "f44":
            name, args = "vf_wino_wgrad", (_ptr(self.x1), _ptr(self.gy), _ptr(dw), _ptr(db), _ptr(db2), _ptr(ws), ws_floats,
                                           *dims, c.mode)
        elif c.C1:
            name, args = "vf_conv1x1_cat_wgrad", (_ptr(self.x1), _ptr(self.x2), c.C1, _ptr(self.gy), _ptr(dw), _ptr(ws),
                                                  ws_floats, *dims)
        else:
            assert not c.db
            name, args = "vf_conv_wgrad", (_ptr(self.x1), _ptr(self.gy), _ptr(dw), _ptr(ws), ws_floats, *dims, c.KS, c.mode)
        if not main:
            rc = getattr(self.lib, name)(*args, _stream())
            torch.cuda.synchronize()
            return rc, None
        row, nblk = (ctypes.c_longlong * 9)(), ctypes.c_int(-1)
        rc = getattr(self.lib, name + "_main")(*args, ctypes.cast(row, ctypes.c_void_p),
                                               ctypes.cast(ctypes.pointer(nblk), ctypes.c_void_p), _stream())
        torch.cuda.synchronize()
        f = dict(zip(("Cout", "Cin", "CoutP", "CinQ", "nslab", "nmain", "first", "nt"), struct.unpack_from("<8i", bytes(row), 40)))
        f.update(ws=row[0], dw=row[1], bsum=row[2], db=row[3], db2=row[4], nblocks=nblk.value, raw=list(row))
        return rc, f


def _assert_row(c, d, f, ws, out):
    """The row a _main entry wrote is the restated plan d."""
    assert (f["nslab"], f["CoutP"], f["CinQ"], f["nt"], f["Cout"], f["Cin"], f["nmain"], f["first"]) == \
           (d["z"], d["CoutP"], d["CinQ"], d["nt"], c.Cout, c.Cin, d["nmain"], 0), (wp.case_id(c), f, d)
    assert f["ws"] == ws.data_ptr() and f["dw"] == out[0].data_ptr()
    assert f["nblocks"] == d["nmain"] + (-(-c.Cout // 64) if c.db else 0)
    if c.family == "f44" and c.db:
        assert f["bsum"] == ws.data_ptr() + 4 * d["z"] * d["slab"] and f["db"] == out[1].data_ptr()      # behind the slabs USED
        assert f["db2"] == (out[2].data_ptr() if c.db == 2 else 0)


# ------------------------------------------------------------------------------------------------ (a) parity per plan class
@pytest.mark.parametrize("c", wp.cases(), ids=wp.case_id)
def test_wgrad_plan_class_vs_fp64(dev, c):
    from view_fusion_amd import ops
    lib = ops._lib.load()
    d = wp.plan(c)
    need = (lib.vf_wino_wgrad_ws_floats(c.S, c.Cin, c.Cout, c.H, c.W) if c.family == "f44" else
            lib.vf_conv_wgrad_ws_floats(c.S, c.Cin, c.Cout, c.H, c.W, c.KS))
    assert need == d["need"] >= d["z"] * d["slab"] + d["tail"]
    t, r64, r32 = _refs(c)
    L = _Launch(lib, dev, c, t)
    scratch, ws = L.outputs(), L.workspace(need)
    rc, f = L.run(scratch, ws, need, main=True)
    assert rc == 0
    _assert_row(c, d, f, ws, scratch)
    out, ws = L.outputs(), L.workspace(need)
    rc, _ = L.run(out, ws, need)
    assert rc == 0
    _judge_all(_label(c, d) + " | " + c.why, c, out, r64, r32)


# ------------------------------------------------------------------------------------------------ (b) hygiene
@pytest.mark.parametrize("c", wp.hygiene_cases(), ids=wp.case_id)
def test_wgrad_writes_every_output_and_stays_inside_its_slabs(dev, c):
    """Neither a slab that is never written nor one that is summed before it is written can hide behind recycled memory:
    dW, db and the workspace start as NaN, the result must be finite and right, the workspace past the z slabs the plan
    uses (F(4x4): past the 256 CoutP bias sums behind them) and the guard untouched, and a second launch bit-identical."""
    from view_fusion_amd import ops
    lib = ops._lib.load()
    d = wp.plan(c)
    t, r64, r32 = _refs(c)
    L = _Launch(lib, dev, c, t)
    runs = []
    for _ in range(2):
        out, ws = L.outputs(), L.workspace(d["need"])
        rc, _ = L.run(out, ws, d["need"])
        assert rc == 0
        used = d["z"] * d["slab"] + d["tail"]
        assert ws.numel() == d["need"] + GUARD and bool(torch.isnan(ws[used:]).all()), "written past the plan's slabs"
        runs.append(out)
    _judge_all(_label(c, d) + " | NaN-filled", c, runs[0], r64, r32)
    for a, b in zip(*runs):
        assert (a is None and b is None) or torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ (c) reduced workspace
@pytest.mark.parametrize("c", wp.clip_cases(), ids=wp.case_id)
def test_wgrad_with_a_smaller_workspace(dev, c):
    """The ABI's contract: a workspace below the preferred size is accepted down to one slab and only lowers z; below
    one slab the entry returns hipErrorInvalidValue and writes nothing."""
    from view_fusion_amd import ops
    lib = ops._lib.load()
    full = wp.plan(c)
    assert full["z"] >= 8
    t, r64, r32 = _refs(c)
    L = _Launch(lib, dev, c, t)
    for slabs in (1, (full["z"] + 1) // 2):
        floats = slabs * full["slab"] + full["tail"]
        d = wp.plan(c, floats)
        assert d["ok"] and d["z"] <= slabs and (slabs > 1 or d["z"] == 1)
        scratch, ws = L.outputs(), L.workspace(full["need"])
        rc, f = L.run(scratch, ws, floats, main=True)
        assert rc == 0
        _assert_row(c, d, f, ws, scratch)
        out, ws = L.outputs(), L.workspace(full["need"])
        rc, _ = L.run(out, ws, floats)
        assert rc == 0
        assert bool(torch.isnan(ws[d["z"] * d["slab"] + d["tail"]:]).all()), "written past the clipped plan's slabs"
        _judge_all(_label(c, d) + f" | ws = {slabs} slab(s)", c, out, r64, r32)
    short = full["slab"] + full["tail"] - 1
    assert not wp.plan(c, short)["ok"]
    for main in (False, True):
        out, ws = L.outputs(), L.workspace(full["need"])
        rc, _ = L.run(out, ws, short, main=main)
        assert rc == INVALID_VALUE, rc
        assert all(bool(torch.isnan(o).all()) for o in out if o is not None) and bool(torch.isnan(ws).all())
        assert torch.equal(out[0].view(torch.int32), torch.full_like(out[0], NAN).view(torch.int32))     # the fill's bit pattern


# ------------------------------------------------------------------------------------------------ (d) the deferred table
# (case, slabs of workspace offered | None: the preferred size, nslab the row must report)
TABLE = ((wp.Case("f44", 33, 32, 64, 8, 8, 3, 0, 0, 2, "F(4x4) row, db + db2"), None, 33),
         (wp.Case("direct", 32, 64, 64, 16, 16, 3, 1, 0, 0, "direct stride-2 row"), None, 64),
         (wp.Case("1x1", 12, 192, 64, 8, 8, 1, 0, 64, 0, "1x1 concatenated row"), None, 3),
         (wp.Case("any", 3, 64, 128, 6, 10, 3, 1, 0, 0, "general-kernel row"), 1, 1))


def test_deferred_table_with_rows_of_all_four_planners(dev):
    """One vf_wino44_reduce_multi launch sums an F(4x4) row (nt = 0, 33 slabs: a second trip of one slab), a direct 9-tap
    row (64 slabs: two whole trips), a concatenated 1x1 row (3 slabs) and a general-kernel row (1 slab): every dW / db
    bitwise equal to the one-call entry's, under the rule, and the same in a second row order."""
    from view_fusion_amd import ops
    from view_fusion_amd.ops.core import _stream
    lib = ops._lib.load()
    assert sorted(n for *_, n in TABLE) == [1, 3, 33, 64]
    items = []
    for c, slabs, nslab in TABLE:
        full = wp.plan(c)
        floats = full["need"] if slabs is None else slabs * full["slab"] + full["tail"]
        d = wp.plan(c, floats)
        assert d["z"] == nslab, (wp.case_id(c), d)
        t, r64, r32 = _refs(c)
        L = _Launch(lib, dev, c, t)
        one, ws1 = L.outputs(), L.workspace(full["need"])
        assert L.run(one, ws1, floats)[0] == 0
        out, ws = L.outputs(), L.workspace(full["need"])
        rc, f = L.run(out, ws, floats, main=True)
        assert rc == 0 and f["nblocks"] > 0
        _assert_row(c, d, f, ws, out)
        assert all(bool(torch.isnan(o).all()) for o in out if o is not None), "a _main entry must not write dW / db"
        items.append((c, d, L, one, out, ws, f, r64, r32))
    for order in ((0, 1, 2, 3), (2, 0, 3, 1)):
        rows, first = [], 0
        for i in order:
            f = items[i][6]
            r = list(f["raw"])
            r[8] = (r[8] & ~0xFFFFFFFF) | first            # `first` = the int32 at byte 64 of the row
            rows.append(r)
            first += f["nblocks"]
        for it in items:
            for o in it[4]:
                if o is not None:
                    o.fill_(NAN)
        table = torch.tensor(rows, dtype=torch.int64).to(dev)
        assert lib.vf_wino44_reduce_multi(ctypes.c_void_p(table.data_ptr()), len(rows), first, _stream()) == 0
        torch.cuda.synchronize()
        for c, d, L, one, out, ws, f, r64, r32 in items:
            for a, b in zip(out, one):
                assert (a is None and b is None) or torch.equal(a, b), (wp.case_id(c), order)
            _judge_all(_label(c, d) + f" | table order {order} | " + c.why, c, out, r64, r32)


# ------------------------------------------------------------------------------------------------ (e) through ops
def _through_ops(dev, c, defer):
    """-> (C-ABI entries logged, [dW, db | None]) of one backward pass of the layer through ops at the default policy."""
    from view_fusion_amd import ops
    t = wp.inputs(c)
    layer = torch.nn.Conv2d(c.Cin, c.Cout, c.KS, stride=2 if c.mode == 1 else 1, padding=c.KS // 2).to(dev)
    x, gy = t["x"].to(dev), t["gy"].to(dev)
    keep_defer = ops.st.WRED_DEFER
    ops.st.WRED_DEFER, ops.st.KERNEL_LOG = defer, []
    try:
        if c.C1:
            y = ops.conv1x1_cat(x[:, :c.C1].contiguous(), x[:, c.C1:].contiguous(), layer)
        else:
            y = ops.conv2d(x, layer, mode={0: "same", 1: "down2", 2: "up2"}[c.mode])
        y.backward(gy)
        torch.cuda.synchronize()
        names = [e[5] for e in ops.st.KERNEL_LOG if e[0] == "conv_wgrad"]
    finally:
        ops.st.WRED_DEFER, ops.st.KERNEL_LOG = keep_defer, None
    return names, [layer.weight.grad, layer.bias.grad]


OPS_CASES = [c for c in wp.cases() if c.why.startswith("bench stride-2")] + [
    wp.Case("1x1", 12, 192, 64, 8, 8, 1, 0, 64, 0, "1x1 concatenated layer"),
    wp.Case("direct", 15, 64, 64, 8, 8, 3, 0, 0, 0, "stride-1 3x3 below the policy edge: S (H/2) (W/2) = 240 < 256"),
    wp.Case("f44", 16, 64, 64, 8, 8, 3, 0, 0, 1, "stride-1 3x3 on the policy edge: S (H/2) (W/2) = 256")]


@pytest.mark.parametrize("c", OPS_CASES, ids=wp.case_id)
def test_wgrad_through_ops_at_the_default_policy(dev, c):
    """ops.conv2d / ops.conv1x1_cat take the entry the policy names (the kernel log says which), deferred (the _main twin
    plus one vf_wino44_reduce_multi) and not, bitwise equal, under the rule.  (8x8 maps hold 16 Winograd tiles a view:
    the edge S (H/2) (W/2) = 255 | 256 lies between S = 15 and S = 16.)"""
    assert len(OPS_CASES) == 6 and c.family == wp.family_of(c.S, c.H, c.W, c.KS, c.mode)
    entry = "vf_conv1x1_cat_wgrad" if c.C1 else wp.ENTRY[c.family]
    d = wp.plan(c)
    t, r64, r32 = _refs(c)
    names, now = _through_ops(dev, c, defer=False)
    assert names == [entry], names
    names, deferred = _through_ops(dev, c, defer=True)
    assert names == [entry + "_main", "vf_wino44_reduce_multi"], names
    assert torch.equal(now[0], deferred[0]) and torch.equal(now[1], deferred[1])
    # (db: the F(4x4) kernel's own sums where it ran, the bias-gradient kernels otherwise -- either way sum(dY))
    full = c._replace(db=1)
    r64b, r32b = (r + [t["gy"].to(r[0].dtype).sum((0, 2, 3))] if len(r) == 1 else r for r in (r64, r32))
    _judge_all(_label(c, d) + " | through ops | " + c.why, full, deferred, r64b[:2], r32b[:2])
