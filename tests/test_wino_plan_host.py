"""The Winograd K-split tail plan on the CPU: tests/wino_plan_ref.py's restatement equals the host functions of
libvf_hip.so over a grid of shapes -- vf_wino_conv_plan, the function the launchers execute, under every workspace, and
the policy's cycle model that reads it --, the plan's invariants hold on that grid, every plan class the SMALL / TINY layers reach
(both directions, S = 1 .. 368) is in wino_plan_ref.cases() -- the list tests/test_gpu_wino_tail_plan.py runs -- and the
comparison rule of those tests rejects two wrong K-splits on the inputs they use."""
import ctypes

import pytest
import torch

import cond_ref as cr
import wino_plan_ref as wp
from conftest import SMALL, TINY

wp.check_env()

GRID_S = range(1, 401)
GRID_CIN = (6, 8, 9, 13, 40, 64, 100, 128, 192, 256, 320, 384, 512, 640)
GRID_COUT = (6, 64, 70, 128, 192, 320, 640)
LIB = {"nested": ("vf_wino_conv_ws_floats", "vf_wino_conv_fill_pct", "vf_wino_supported"),
       "f44": ("vf_wino44_conv_ws_floats", "vf_wino44_conv_fill_pct", "vf_wino44_supported")}


@pytest.fixture(scope="module")
def lib():
    from view_fusion_amd import _lib
    return _lib.load()


def _grid(kernel):
    for W in wp.MAPS[kernel]:
        for S in GRID_S:
            for Cin in GRID_CIN:
                for Cout in GRID_COUT:
                    yield S, Cin, Cout, W


@pytest.mark.parametrize("kernel", wp.KERNELS)
def test_restatement_equals_the_library_and_the_plan_keeps_its_invariants(lib, kernel):
    f_ws, f_fill, _ = (getattr(lib, n) for n in LIB[kernel])
    tiles = ctypes.c_int(0)
    n = 0
    for S, Cin, Cout, W in _grid(kernel):
        d = wp.describe(kernel, S, Cin, Cout, W, W)
        T, nch, nfull, R, split, per = (d[k] for k in ("T", "nch", "nfull", "R", "split", "per"))
        at = (kernel, S, Cin, Cout, W, d)
        # the restatement is the library's plan
        assert f_ws(S, Cin, Cout, W, W) == d["parts"] * wp.PART_FLOATS[kernel] == wp.ws_floats(kernel, S, Cin, Cout, W, W), at
        pct = f_fill(S, Cin, Cout, W, W, ctypes.byref(tiles))
        assert (pct, tiles.value) == wp.fill_pct(kernel, S, Cin, Cout, W, W) and tiles.value == T, at
        # invariants
        assert nfull + R == T and 1 <= split <= 8, at
        if split > 1:
            assert nfull % wp.SLOTS == 0 and per >= 4 and 0 < R < wp.SLOTS, at
        else:
            assert R == 0 and d["parts"] == 0, at
        rg = wp.ranges(nch, split)
        assert len(rg) == split and all(a < b for a, b in rg), at                       # no empty range
        assert rg[0][0] == 0 and rg[-1][1] == nch and all(rg[i][1] == rg[i + 1][0] for i in range(split - 1)), at
        assert d["last"] == rg[-1][1] - rg[-1][0] and 0 < d["last"] <= per, at
        if T // wp.SLOTS >= 3 or T % wp.SLOTS == 0:
            assert split == 1, at
        n += 1
    assert n == len(wp.MAPS[kernel]) * len(GRID_S) * len(GRID_CIN) * len(GRID_COUT)


def _ask(lib, kernel, S, Cin, Cout, W, mode, has_ws, ws, out=None):
    """vf_wino_conv_plan -> (rc, dict of PLAN_FIELDS)."""
    out = (ctypes.c_int * 8)() if out is None else out
    rc = lib.vf_wino_conv_plan(wp.KIND[kernel], S, Cin, Cout, W, W, mode, has_ws, ws, ctypes.cast(out, ctypes.c_void_p))
    return rc, dict(zip(wp.PLAN_FIELDS, out))


@pytest.mark.parametrize("kernel", wp.KERNELS)
def test_the_plan_query_equals_the_restatement_under_every_workspace(lib, kernel):
    """vf_wino_conv_plan -- the function the launchers execute -- field for field, with the workspace at the priced size,
    one float short of it (the plain grid), at zero and absent; the unclamped plan is the one *_conv_ws_floats prices."""
    f_ws = getattr(lib, LIB[kernel][0])
    out = (ctypes.c_int * 8)()
    n = split = 0
    for S, Cin, Cout, W in _grid(kernel):
        d = wp.describe(kernel, S, Cin, Cout, W, W)
        need = f_ws(S, Cin, Cout, W, W)
        assert need == d["parts"] * wp.PART_FLOATS[kernel], (kernel, S, Cin, Cout, W)
        for has_ws, ws in ((1, need), (1, need - 1), (1, 0), (0, need), (0, 0)):
            if ws < 0:
                continue
            want = wp.launch_plan(kernel, S, Cin, Cout, W, W, has_ws, ws)
            assert _ask(lib, kernel, S, Cin, Cout, W, 0, has_ws, ws, out) == (0, want), (kernel, S, Cin, Cout, W, has_ws, ws)
            if (has_ws, ws) == (1, need):                   # the priced workspace runs the plan describe() states
                assert all(want[k] == d[k] for k in ("T", "nch", "nfull", "split", "per")), (kernel, S, Cin, Cout, W)
                assert (want["conv_grid"] - want["npers"]) * wp.PART_FLOATS[kernel] == need
                assert _ask(lib, kernel, S, Cin, Cout, W, 2, 1, need, out) == (0, want)     # the mode plays no part
            elif d["split"] > 1:                            # anything less: every tile whole, no fix-up
                assert (want["nfull"], want["split"], want["fixup_grid"]) == (d["T"], 1, 0)
                assert want["conv_grid"] == want["npers"] == min(d["T"], wp.SLOTS)
        split += d["split"] > 1
        n += 1
    assert n == len(wp.MAPS[kernel]) * len(GRID_S) * len(GRID_CIN) * len(GRID_COUT) and split > 0


def test_the_plan_query_refuses_what_the_entries_refuse(lib):
    out = (ctypes.c_int * 8)()
    for kernel in wp.KERNELS:
        for H in (4, 8, 12, 16, 32, 48, 64, 128):
            for W in (8, 16, 32, 64, 128):
                for mode in (0, 1, 2, 4):
                    rc = lib.vf_wino_conv_plan(wp.KIND[kernel], 2, 64, 64, H, W, mode, 0, 0, ctypes.cast(out, ctypes.c_void_p))
                    assert (rc == 0) == wp.supported(kernel, H, W, mode), (kernel, H, W, mode, rc)
                    assert rc in (0, 1)
        W = wp.MAPS[kernel][-1]
        assert _ask(lib, kernel, 2, 64, 64, W, 0, 0, 0)[0] == 0
        assert _ask(lib, kernel, 0, 64, 64, W, 0, 0, 0)[0] == 1 and _ask(lib, kernel, -1, 64, 64, W, 0, 0, 0)[0] == 1
        assert lib.vf_wino_conv_plan(wp.KIND[kernel], 2, 64, 64, W, W, 0, 0, 0, None) == 1
    for kind in (0, 3):
        assert lib.vf_wino_conv_plan(kind, 2, 64, 64, 32, 32, 0, 0, 0, ctypes.cast(out, ctypes.c_void_p)) == 1


def test_policy_cycles_equal_the_restated_cost_model(lib):
    """ops.policy._wino_cycles reads the plan from vf_wino_conv_plan; the figure is the restated model's, bit for bit."""
    from view_fusion_amd.ops import policy
    assert {k: policy._WINO_COST[wp.KIND[k]] for k in wp.KERNELS} == wp.WINO_COST
    n = 0
    for kernel in wp.KERNELS:
        for S, Cin, Cout, W in _grid(kernel):
            assert policy._wino_cycles(wp.KIND[kernel], S, Cin, Cout, W, W) == wp.cycles(kernel, S, Cin, Cout, W, W), (kernel, S, Cin, Cout, W)
            n += 1
    assert n == 6 * len(GRID_S) * len(GRID_CIN) * len(GRID_COUT)


def test_abi_has_the_plan_entry(lib):
    """The header declaration, the ctypes signature and the definition agree in argument count."""
    import os
    import re
    from view_fusion_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "vf_hip.h")).read()
    source = open(os.path.join(root, "view_fusion_amd", "csrc", "winograd24.hip")).read()
    arity = lambda m: len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
    decl = re.search(r"\bint\s+vf_wino_conv_plan\s*\(([^;{]*)\)\s*;", header)
    defn = re.search(r"\bint\s+vf_wino_conv_plan\s*\(([^;{]*)\)\s*\{", source)
    assert decl, "vf_wino_conv_plan is not declared in include/vf_hip.h"
    assert defn, "vf_wino_conv_plan is not defined in csrc/winograd24.hip"
    assert arity(decl) == arity(defn) == len(_lib.SIGNATURES["vf_wino_conv_plan"]) == 10 and hasattr(lib, "vf_wino_conv_plan")
    I_, L_, P_ = _lib._I, _lib._L, _lib._P
    assert _lib.SIGNATURES["vf_wino_conv_plan"] == [I_] * 8 + [L_, P_]


def test_shape_predicates_equal_the_library(lib):
    for kernel in wp.KERNELS:
        f_sup = getattr(lib, LIB[kernel][2])
        for H in (4, 8, 12, 16, 32, 48, 64, 128):
            for W in (4, 8, 16, 32, 64, 128):
                for mode in (0, 1, 2):
                    assert bool(f_sup(H, W, mode)) == wp.supported(kernel, H, W, mode), (kernel, H, W, mode)
    for W in wp.MAPS["nested"]:
        for S in (1, 2, 3, 5, 6, 9, 12, 16, 17, 40):
            for Cin in GRID_CIN:
                for Cout in (32, 64, 96, 128, 160, 320, 640, 70):
                    for mode in (0, 2):
                        for g in (32, 8):
                            assert bool(lib.vf_wino_conv_gn_fusable(S, Cin, Cout, W, W, mode, g)) == \
                                wp.gn_fusable(S, Cin, Cout, W, W, mode, g), (S, Cin, Cout, W, mode, g)


def _model_layers():
    """(Cin, Cout, H, mode) of every stride-1 3x3 conv of the SMALL and TINY networks, from their own geometry marks."""
    from view_fusion_amd import UNet
    out = set()
    for hp in (SMALL, TINY):
        net = UNet(**hp)
        for m in net.modules():
            geom = getattr(m, "_vf_geom", None)
            if isinstance(m, torch.nn.Conv2d) and geom is not None and m.kernel_size == (3, 3) and geom[1] in ("same", "up2"):
                out.add((m.in_channels, m.out_channels, hp["image_size"] >> geom[0], geom[1]))
    return sorted(out)


def test_every_class_the_models_reach_is_in_the_case_list(lib):
    layers = _model_layers()
    assert any(h == 64 for _, _, h, _ in layers) and any(m == "up2" for *_, m in layers) and len(layers) >= 20
    reached = {}
    for Cin, Cout, H, mode in layers:
        for kernel in wp.KERNELS:
            if not getattr(lib, LIB[kernel][2])(H, H, wp_mode(mode)):
                continue
            assert wp.supported(kernel, H, H, wp_mode(mode))
            for ci, co in ((Cin, Cout), (Cout, Cin)):                 # the conv and its dgrad
                for S in range(1, wp.S_MAX + 1):
                    reached.setdefault(wp.plan_class(kernel, S, ci, co, H, H), (S, ci, co))
    covered = wp.covered_classes()
    print()
    print("CLASS | kernel | map | split | short last | first reached at (S, Cin, Cout) | in cases()")
    for cls in sorted(set(reached) | covered):
        at = reached.get(cls)
        print(f"CLASS | {cls[0]} | {cls[1]} | {cls[2]} | {'yes' if cls[3] else 'no'} | {at if at else 'not by the models'} | "
              f"{'yes' if cls in covered else 'NO'}")
    for row in wp.case_table():
        print("RULE | " + " | ".join(str(v) for v in row))
    print(f"reachable classes {len(reached)}, covered {len(set(reached) & covered)}; cases {len(wp.cases())}")
    assert set(reached) <= covered, sorted(set(reached) - covered)


def wp_mode(mode):
    return {"same": 0, "up2": 2}[mode]


def test_case_list_is_deterministic_and_holds_the_named_classes():
    cs = wp.cases()
    wp._enumerate.cache_clear()
    assert wp.cases() == cs and len({wp.case_id(c) for c in cs}) == len(cs)
    D = [(c, wp.describe(c.kernel, c.S, c.Cin, c.Cout, c.H, c.H)) for c in cs]
    short = lambda d: d["split"] > 1 and d["last"] < d["per"]
    has = lambda kernel, W, pred, mode="same": any(c.kernel == kernel and c.H == W and c.mode == mode and pred(d) for c, d in D)
    assert has("f44", 64, short) and has("f44", 32, short)
    assert has("f44", 64, lambda d: d["split"] == 4)
    assert has("nested", 64, lambda d: d["split"] == 4) and has("nested", 64, lambda d: d["split"] == 6)
    for kernel in wp.KERNELS:
        for W in wp.MAPS[kernel]:
            assert has(kernel, W, lambda d: d["parts"] > 256), (kernel, W)
            assert has(kernel, W, lambda d: d["nfull"] == 256 and d["split"] > 1), (kernel, W)
            assert has(kernel, W, lambda d: d["nfull"] == 512 and d["split"] > 1), (kernel, W)
            assert has(kernel, W, short, "up2"), (kernel, W)
            assert any(c.kernel == kernel and c.H == W and c.Cin % 8 and d["split"] > 1 for c, d in D), (kernel, W)
    ragged3 = lambda d: d["T"] // 256 >= 3 and d["R"] == 0 and d["T"] % 256 and d["nfull"] % 8
    assert has("f44", 32, ragged3) and has("nested", 32, ragged3) and has("nested", 16, ragged3) and has("nested", 8, ragged3)
    for r in (1, 2, 3):
        assert any(c.kernel == "nested" and c.H == 8 and c.S > 4 and c.S % 4 == r and d["split"] >= 5 for c, d in D)
    # what the enumeration reports as not producible is not producible: T is a multiple of the groups per view
    missing = {(k, W, rule) for k, W, rule, hit in wp.case_table() if hit == "not producible"}
    assert ("nested", 64, "3+rounds ragged") in missing and ("f44", 64, "3+rounds ragged") in missing
    assert all(rule in ("3+rounds ragged", "R=1", "R=255", "T%256=255") for _, _, rule in missing), missing
    assert all((k, W, "R=255") in missing for k in wp.KERNELS for W in wp.MAPS[k])      # (see wino_plan_ref.SPECIALS)
    assert len(wp.hygiene_cases()) == 8 and len(wp.gn_cases()) >= 3 * 14


def test_cases_stay_small():
    """A case, its CPU references included, has to stay at a few seconds: bound the multiply-adds of its forward.  (The
    largest is a split tail behind two full rounds of F(4x4) tiles: 520 tiles x 512 pixels x 64 channels x 10 chunks,
    1.2e10 -- two seconds of float64 forward + backward on eight cores.)"""
    for c in wp.cases():
        assert 9 * c.S * c.Cin * c.Cout * c.H * c.H <= 1.5e10, wp.case_id(c)


# ---------------------------------------------------------------------------------------- the inputs discriminate
@pytest.mark.parametrize("kernel", wp.KERNELS)
def test_wrong_k_splits_fail_the_rule(kernel):
    """A K-split that drops the last chunk of the short last range, and one whose ranges start one chunk late, both FAIL
    the rule of the GPU tests on the GPU tests' inputs; the right split passes it."""
    c = next(c for c in wp.cases() if c.kernel == kernel and c.mode == "same" and c.Cin % 8 == 0
             and (lambda d: d["split"] > 1 and d["last"] < d["per"])(wp.describe(kernel, c.S, c.Cin, c.Cout, c.H, c.H)))
    d = wp.describe(kernel, c.S, c.Cin, c.Cout, c.H, c.H)
    t = wp.inputs(c)
    (r64,), (r32,) = wp.conv_ref(t, c.mode, torch.float64, backward=False), wp.conv_ref(t, c.mode, torch.float32, backward=False)
    rg = wp.ranges(d["nch"], d["split"])
    good = wp.conv_ksplit(t, rg)
    dropped = wp.conv_ksplit(t, rg[:-1] + [(rg[-1][0], rg[-1][1] - 1)])
    late = wp.conv_ksplit(t, [(a + 1, min(b + 1, d["nch"])) for a, b in rg])
    for name, y, want in (("right split", good, True), ("last chunk dropped", dropped, False), ("c0 one chunk late", late, False)):
        err, e, b, ok = cr.judge(y, r64, r32, wp.TOL[kernel])
        print(f"{wp.case_id(c)} {name}: err {err:.3e}  e {e:.3e}  bound {b:.3e}")
        assert ok == want, (name, err, b)


def test_tuning_overrides_fail_loudly():
    """(On a copy of the environment: the library reads the variables once per process, so no test may set them.)"""
    for k in wp.ENV:
        with pytest.raises(RuntimeError, match=k):
            wp.check_env({k: "3.0"})
    wp.check_env({})
    wp.check_env()
