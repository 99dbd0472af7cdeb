"""The weight-gradient slab plans on the CPU: tests/wgrad_plan_ref.py's restatement of the three *_ws_floats functions
equals the host functions of libvf_hip.so over the whole domain, the workspace ops allocates never clips a plan, every
plan class the SMALL / TINY layers reach (S = 1 .. 368) is in wgrad_plan_ref.cases() -- the list
tests/test_gpu_wgrad_plan.py runs -- every case stays under the reference-cost cap, and the comparison rule of those
tests rejects five wrong slab decompositions on the inputs they use.

vf_conv_wgrad_ws_floats over-allocates for KS = 3 by design: it takes a CEILING over 32-channel ci tiles where the
launcher takes a floor over 64-channel ones (the BIG kernel) or a floor over 32-channel ones (stride 2).  What is
asserted is need >= z slab, never equality.

The launch plan itself (z, CoutP, CinQ) is not visible on the host; tests/test_gpu_wgrad_plan.py pins it to the row every
*_main entry writes."""
import itertools

import numpy as np
import pytest
import torch

import cond_ref as cr
import wgrad_plan_ref as wp
from conftest import SMALL, TINY

wp.check_env()

WALK_S = (1, 6, 12, 48, 96, 368)


@pytest.fixture(scope="module")
def lib():
    from view_fusion_amd import _lib
    return _lib.load()


def _maps():
    out = [("conv", W, W, 3) for W in wp.DIRECT_MAPS[0]] + [("conv", W, W, 1) for W in wp.ONE_MAPS]
    out += [("conv", H, W, KS) for H, W, KS, _ in wp.ANY_SHAPES if not wp.square_pow2(H, W)]
    return out + [("f44", W, W, 3) for W in wp.F44_MAPS]


def test_ws_floats_restatements_equal_the_library(lib):
    """On the whole domain: S = 1 .. 368 x every channel pair x every map of the enumeration (7.6 M shapes)."""
    S, Ci, Co = wp._grid()
    shape = (S.size, Ci.size, Co.size)
    pts = list(itertools.product(S.ravel().tolist(), Ci.ravel().tolist(), Co.ravel().tolist()))
    n = 0
    for kind, H, W, KS in _maps():
        if kind == "conv":
            f = lib.vf_conv_wgrad_ws_floats
            want = wp.ws_conv(S, Ci, Co, H, W, KS)
            got = [f(s, ci, co, H, W, KS) for s, ci, co in pts]
        else:
            f = lib.vf_wino_wgrad_ws_floats
            want = wp.ws_f44(S, Ci, Co, H, W)
            got = [f(s, ci, co, H, W) for s, ci, co in pts]
        bad = np.nonzero(np.array(got, dtype=np.int64) != np.broadcast_to(want, shape).ravel())[0]
        assert bad.size == 0, (kind, H, W, KS, pts[bad[0]], got[bad[0]], int(np.broadcast_to(want, shape).ravel()[bad[0]]))
        n += len(got)
    assert n == len(_maps()) * wp.S_MAX * len(wp.CHANNELS) ** 2 and len(_maps()) == 19


def test_shape_predicates_and_the_policy_edge_equal_the_library(lib):
    from view_fusion_amd.ops import policy
    for H in (4, 8, 12, 16, 32, 48, 64, 128):
        for W in (4, 8, 16, 32, 64, 128):
            for mode in (0, 1, 2):
                assert bool(lib.vf_wino_wgrad_supported(H, W, mode)) == (H == W and W in wp.F44_MAPS and mode in wp.F44_MODES)
                for S in (1, 3, 4, 15, 16, 63, 64, 255, 256):
                    assert bool(policy.use_winograd_wgrad(S, 64, 64, H, W, 3, mode)) == wp.use_winograd_wgrad(S, H, W, 3, mode)
    assert policy.st.WINO_WGRAD_MIN_TILES == wp.WINO_WGRAD_MIN_TILES
    assert not policy.use_winograd_wgrad(255, 64, 64, 16, 16, 1, 0)
    for C in range(1, 1100):
        assert int(wp.wgrad1_tile(C)) == (128 if 5 * ((C + 127) // 128 * 128) <= 6 * ((C + 63) // 64 * 64) else 64)


def _plans():
    """(label, plan over the whole domain) of every (family, map, mode) of the enumeration."""
    S, Ci, Co = wp._grid()
    for mode, maps in wp.DIRECT_MAPS.items():
        for W in maps:
            yield ("direct", W, mode), wp.plan_direct(S, Ci, Co, W, mode)
    for W in wp.ONE_MAPS:
        yield ("1x1", W, 0), wp.plan_1x1(S, Ci, Co, W)
    for W in wp.F44_MAPS:
        for mode in wp.F44_MODES:
            yield ("f44", W, mode), wp.plan_f44(S, Ci, Co, W, mode)
    for H, W, KS, mode in wp.ANY_SHAPES:
        yield ("any", H, W, KS, mode), wp.plan_any(S, Ci, Co, H, W, KS, mode)


def test_the_workspace_ops_allocates_never_clips_the_plan_and_the_plans_keep_their_invariants():
    """On the whole domain: *_ws_floats (what ops allocates) >= z slab (+ 256 CoutP for F(4x4)) of the restated launch
    plan; passing exactly that size back leaves the plan unchanged; the slices tile [0, units) with no empty slice."""
    S, Ci, Co = wp._grid()
    for label, d in _plans():
        units, z, per, last = (np.broadcast_to(d[k], (S.size, Ci.size, Co.size)) for k in ("units", "z", "per", "last"))
        assert np.all(d["need"] >= d["z"] * d["slab"] + d["tail"]), label
        assert np.all((z >= 1) & (z <= units) & (per >= 1) & (last >= 1) & (last <= per) & ((z - 1) * per + last == units)), label
        if label[0] == "1x1":
            assert np.all((per >= 4) | (z == 1)), label
        if label[0] == "direct":
            clipped = wp.plan_direct(S, Ci, Co, label[1], label[2], ws=d["need"])
        elif label[0] == "1x1":
            clipped = wp.plan_1x1(S, Ci, Co, label[1], ws=d["need"])
        elif label[0] == "f44":
            clipped = wp.plan_f44(S, Ci, Co, label[1], label[2], ws=d["need"])
        else:
            clipped = wp.plan_any(S, Ci, Co, *label[1:], ws=d["need"])
        assert np.all(clipped["ok"]) and np.all(clipped["z"] == d["z"]) and np.all(clipped["per"] == d["per"]), label


def test_clipped_plans():
    """ws_floats below the preferred size: z = min(preferred, floor(ws / slab)), then per and z recomputed; below one slab
    the launch is refused."""
    for c in wp.clip_cases():
        d = wp.plan(c)
        assert d["z"] >= 8
        one = wp.plan(c, d["slab"] + d["tail"])
        assert one["ok"] and one["z"] == 1 and one["per"] == d["units"] and one["last"] == d["units"]
        hz = (d["z"] + 1) // 2
        h = wp.plan(c, hz * d["slab"] + d["tail"])
        assert h["ok"] and h["z"] <= hz and h["per"] == -(-d["units"] // hz) and (h["z"] - 1) * h["per"] + h["last"] == d["units"]
        assert not wp.plan(c, d["slab"] + d["tail"] - 1)["ok"]


def _model_layers():
    """(Cin, Cout, H, KS, mode, C1 | 0) of every conv of the SMALL and TINY networks, from their own geometry marks; C1:
    the channels of the decoder activation in front of a residual 1x1 conv that reads [x | skip]."""
    from view_fusion_amd import UNet
    out = set()
    for hp in (SMALL, TINY):
        net = UNet(**hp)
        cat = {}
        ch = net.mid[-1].res_block.block2["block"]["3"].out_channels
        for layer in net.ups:
            rb = getattr(layer, "res_block", None)
            if rb is not None:
                if isinstance(rb.res_conv, torch.nn.Conv2d):
                    cat[rb.res_conv] = ch
                ch = rb.block2["block"]["3"].out_channels
        for m in net.modules():
            geom = getattr(m, "_vf_geom", None)
            if isinstance(m, torch.nn.Conv2d) and geom is not None:
                mode = {"same": 0, "down2": 1, "up2": 2}[geom[1]]
                out.add((m.in_channels, m.out_channels, hp["image_size"] >> geom[0], m.kernel_size[0], mode, cat.get(m, 0)))
    return sorted(out)


def test_every_class_the_models_reach_is_in_the_case_list():
    layers = _model_layers()
    assert any(ks == 1 and c1 for *_, ks, _, c1 in layers) and {m for *_, m, _ in layers} == {0, 1, 2} and len(layers) >= 30
    assert {c for l in layers for c in l[:2]} <= set(wp.CHANNELS), "a model layer outside the enumeration's channel domain"
    reached = {}
    for Cin, Cout, H, KS, mode, C1 in layers:
        for S in WALK_S:
            fam = wp.family_of(S, H, H, KS, mode)
            # (a concatenation that the GroupNorm in front cannot fuse is materialised: both routes count; F(4x4): the
            # bias sums ride along or not, depending on what the GroupNorm backward has already summed)
            variants = [(c1, db) for c1 in {0, C1 if C1 % 64 == 0 else 0} for db in ((0, 1, 2) if fam == "f44" else (0,))]
            for c1, db in variants:
                c = wp.Case(fam, S, Cin, Cout, H, H, KS, mode, c1, db, "")
                for cls in wp.plan_classes(c) + [wp.reduce_class(c)]:
                    reached.setdefault(cls, wp.case_id(c))
    covered = wp.covered_classes()
    print()
    for cls in sorted(set(reached) | covered, key=str):
        print(f"CLASS | {' | '.join(str(v) for v in cls)} | first reached at {reached.get(cls, 'not by the models')} | "
              f"{'in cases()' if cls in covered else 'NOT COVERED'}")
    print(f"reached classes {len(reached)}, covered {len(set(reached) & covered)} of them; classes in cases() {len(covered)}; "
          f"cases {len(wp.cases())}")
    assert {"direct", "1x1", "f44"} <= {cls[0].split()[0] for cls in reached}
    assert set(reached) <= covered, sorted(set(reached) - covered, key=str)


def test_case_list_is_deterministic_capped_and_holds_the_named_cases():
    cs = wp.cases()
    wp._enumerate.cache_clear()
    wp._order.cache_clear()
    assert wp.cases() == cs and len({wp.case_id(c) for c in cs}) == len(cs)
    print()
    for c in sorted(cs, key=wp.cost)[-5:]:
        print(f"COST | {wp.case_id(c)} | {wp.cost(c):.2e} | {c.why}")
    for c in cs:
        # (a class whose cheapest representative is above the cap fails here: it is not dropped)
        assert wp.cost(c) <= wp.CAP_MACS, (wp.case_id(c), wp.cost(c), c.why)
        if c.family == "f44":
            assert c.KS == 3 and c.H == c.W and c.W in wp.F44_MAPS and c.mode in wp.F44_MODES
        else:
            assert (c.family != "any") == wp.direct_specialised(c.KS, c.H, c.W, c.mode) and (c.family == "1x1") <= (c.KS == 1)
        assert not c.C1 or (c.KS == 1 and c.C1 % 64 == 0 and 0 < c.C1 < c.Cin)
    D = [(c, wp.plan(c)) for c in cs]
    assert any(c.family == "direct" and c.Cout == 6 for c, _ in D) and any(c.family == "direct" and c.Cin == 6 for c, _ in D)
    assert any(c.family == "direct" and c.mode != 1 and d["CinQ"] == 96 for c, d in D)
    assert {(d["tm"], d["tn"]) for c, d in D if c.family == "1x1"} == {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert any(c.family == "direct" and d["half"] and d["z"] > 1 for c, d in D)
    assert any(c.family == "any" and d["partial_step"] and d["last"] < d["per"] for c, d in D)
    for full, scaled in wp.BENCH_PLANS:            # the stand-ins of the bench step's stride-2 layers run the bench's plan
        a, b = (wp.plan(wp.Case("direct", S, Cin, Cout, H, H, 3, 1, 0, 0, "")) for S, Cin, Cout, H in (full, scaled))
        assert all(a[k] == b[k] for k in ("units", "z", "per", "last", "half")), (full, scaled)
        assert any(c.family == "direct" and (c.S, c.Cin, c.Cout, c.H) == scaled and c.mode == 1 for c in cs)
    assert [(wp.plan(wp.Case("direct", 96, ci, co, h, h, 3, 1, 0, 0, ""))[k]) for (_, ci, co, h), _ in wp.BENCH_PLANS
            for k in ("units", "z", "per")] == [768, 256, 3, 192, 64, 3, 48, 24, 2]
    # every class of the slab sum: one slab, one trip with 2-4 / 5-32 slabs, a second trip (33: one slab in it), whole
    # trips, ragged trips -- for each of the three bodies (nt = 0 | 1 | 9), with a whole and a ragged last workgroup
    assert {wp.reduce_class(c) for c in cs} == {("reduce", nt, b, r) for nt in (0, 1, 9) for b in wp.NSLAB_BUCKETS for r in (False, True)}
    assert len(wp.hygiene_cases()) >= 12 and len(wp.clip_cases()) == 4


def test_reduce_trips_cover_every_slab_once():
    for n in list(range(1, 140)) + [255, 256, 257, 512]:
        trips = wp.reduce_trips(n)
        flat = sorted(s for g in trips for t in g for s in t)
        assert flat == list(range(n)), n
        assert all(len(g) == len(range(gi, n, 32)) for gi, g in enumerate(trips))


# ---------------------------------------------------------------------------------------- the inputs discriminate
@pytest.mark.parametrize("family", wp.FAMILIES)
def test_slab_model_passes_the_rule_and_every_mutant_fails_it(family):
    """For every case: the slab decomposition evaluated in fp32 on the CPU (one partial per slice over exactly that
    slice's units, the slab sum's grouping and order) PASSES the rule of the GPU tests at tol = 1e-4 / 2e-5, and each
    applicable wrong decomposition -- last unit of the last slice dropped, every slice range one unit late, one slab
    skipped by the sum, image S - 1 read in place of the missing image of a half-empty 8x8 tile, the padded channel rows
    folded into channel 0 -- FAILS it on dW."""
    n = 0
    print()
    for c in wp.cases():
        if c.family != family:
            continue
        d, t = wp.plan(c), wp.inputs(c)
        r64, r32 = wp.wgrad_ref(t, c, torch.float64), wp.wgrad_ref(t, c, torch.float32)
        cache = {}
        got = wp.wgrad_slabs(t, c, d, cache=cache)
        for name, a, b64, b32, tol in zip(wp.NAMES, got, r64, r32, wp.tols(c)):
            err, e, bound, ok = cr.judge(a, b64, b32, tol)
            assert ok, (wp.case_id(c), name, err, bound)
        line = [f"MUTANT | {wp.case_id(c)} | slabs {cr.err(got[0], r64[0]):.1e}"]
        for m in wp.MUTANTS:
            if not wp.mutant_applies(c, d, m):
                continue
            err, e, bound, ok = cr.judge(wp.wgrad_slabs(t, c, d, mutate=m, cache=cache)[0], r64[0], r32[0], wp.TOL_DW)
            line.append(f"{m} {err:.1e}")
            assert not ok, (wp.case_id(c), m, err, bound)
            n += 1
        print(" | ".join(line))
    assert n >= 3 * sum(c.family == family for c in wp.cases())


def test_policy_override_fails_loudly():
    """(On a copy of the environment: ops reads the variable once per process, so no test may set it.)"""
    for k in wp.ENV:
        with pytest.raises(RuntimeError, match=k):
            wp.check_env({k: "64"})
    wp.check_env({})
    wp.check_env()
