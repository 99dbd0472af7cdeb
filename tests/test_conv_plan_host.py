"""The forward / dgrad launch plans of the direct convolutions on the CPU: tests/conv_plan_ref.py's restatement equals the
host functions of libvf_hip.so over the whole domain -- vf_conv_fwd_ws_floats exactly, all eight fields of
vf_conv_fwd_plan with the workspace at the priced size, at one slab, at ks - 1 slabs and absent -- the priced workspace
always holds the slabs the launch writes, every plan class the SMALL / TINY layers reach (S = 1 .. 368, forward and dgrad
direction) is in conv_plan_ref.cases() -- the list tests/test_gpu_conv_plan.py runs -- every case stays under the
reference-cost cap, and the comparison rule of those tests rejects six wrong split decompositions on the inputs they use.

vf_conv_fwd_plan is the function the launchers execute (csrc/conv.hip: conv_fwd_impl runs conv_fwd_plan and launches what
it says), so pinning it pins the launch."""
import concurrent.futures
import ctypes
import itertools
import multiprocessing
import os

import numpy as np
import pytest
import torch

import cond_ref as cr
import conv_plan_ref as cp

cp.check_env()


@pytest.fixture(scope="module")
def lib():
    from view_fusion_amd import _lib
    return _lib.load()


def _points():
    S, Ci, Co = cp._grid()
    shape = (S.size, Ci.size, Co.size)
    s, ci, co = (np.broadcast_to(a, shape).ravel() for a in (S, Ci, Co))
    return shape, s, ci, co


def _query(lib, s, ci, co, H, W, KS, mode, C1, C1o, gn, has_ws, ws):
    """vf_conv_fwd_plan at every point -> (n, 8) int32."""
    n = s.size
    out = np.full((n, 8), -1, dtype=np.int32)
    base = out.ctypes.data
    rep = itertools.repeat
    rcs = list(map(lib.vf_conv_fwd_plan, s.tolist(), ci.tolist(), co.tolist(), rep(H), rep(W), rep(KS), rep(mode), rep(C1), rep(C1o),
                   rep(gn), rep(has_ws), np.broadcast_to(ws, (n,)).tolist(), range(base, base + 32 * n, 32)))
    assert not any(rcs), "vf_conv_fwd_plan refused a shape of the sweep"
    return out


def _want(d, shape):
    return np.stack([np.broadcast_to(d[k], shape).ravel() for k in cp.FIELDS], 1)


def _compare(got, d, shape, pts, label):
    want = _want(d, shape)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (label, tuple(int(p[bad[0]]) for p in pts), dict(zip(cp.FIELDS, got[bad[0]].tolist())),
                           dict(zip(cp.FIELDS, want[bad[0]].tolist())))


def _check_row(row):
    """One (H, W, KS, mode) row of the sweep -> number of shapes checked.  (A top-level function: the rows run in worker
    processes, the library's host functions being pure.)"""
    from view_fusion_amd import _lib
    lib = _lib.load()
    H, W, KS, mode = label = row
    shape, s, ci, co = _points()
    S, Ci, Co = cp._grid()
    need = np.broadcast_to(cp.ws_floats(S, Ci, Co, H, W, KS), shape).ravel()
    got = np.array(list(map(lib.vf_conv_fwd_ws_floats, s.tolist(), ci.tolist(), co.tolist(), itertools.repeat(H),
                            itertools.repeat(W), itertools.repeat(KS))), dtype=np.int64)
    bad = np.nonzero(got != need)[0]
    assert bad.size == 0, (label, int(s[bad[0]]), int(ci[bad[0]]), int(co[bad[0]]), int(got[bad[0]]), int(need[bad[0]]))
    d = cp.plan_arrays(S, Ci, Co, H, W, KS, mode)
    out_floats = np.broadcast_to(d["out_floats"], shape).ravel()
    ks = np.broadcast_to(d["ks"], shape).ravel()
    assert np.all((ks == 1) | (ks * out_floats <= need)), label
    assert np.all(np.broadcast_to(d["ks"] <= d["pks"], shape)), (label, "the launch never wants more slabs than the price")
    _compare(_query(lib, s, ci, co, H, W, KS, mode, 0, 0, 0, 1, need), d, shape, (s, ci, co), label + ("priced",))
    for name, ws in (("one slab", out_floats), ("ks - 1 slabs", np.maximum(ks - 1, 1) * out_floats)):
        dd = cp.plan_arrays(S, Ci, Co, H, W, KS, mode, ws=ws.reshape(shape))
        assert np.all(np.broadcast_to(dd["ks"], shape).ravel() == (1 if name == "one slab" else np.maximum(ks - 1, 1)))
        _compare(_query(lib, s, ci, co, H, W, KS, mode, 0, 0, 0, 1, ws), dd, shape, (s, ci, co), label + (name,))
    dd = cp.plan_arrays(S, Ci, Co, H, W, KS, mode, ws=None)
    assert np.all(dd["ks"] == 1)
    _compare(_query(lib, s, ci, co, H, W, KS, mode, 0, 0, 0, 0, 0), dd, shape, (s, ci, co), label + ("absent",))
    return s.size


def test_ws_floats_and_the_plan_equal_the_library_on_the_whole_sweep(lib):
    """S = 1 .. 368 x every channel pair x every map of the launch tables and ANY_SHAPES (10.9 M shapes): the price, and the
    plan at four workspace sizes; the priced workspace holds every slab the launch writes."""
    workers = min(8, len(os.sched_getaffinity(0)))
    if workers > 1:
        with concurrent.futures.ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as pool:
            n = sum(pool.map(_check_row, cp.rows()))
    else:
        n = sum(_check_row(r) for r in cp.rows())
    assert n == len(cp.rows()) * cp.S_MAX * len(cp.CHANNELS) ** 2 and len(cp.rows()) == 31


def test_groupnorm_concatenation_and_split_output_plans_equal_the_library(lib):
    """vf_conv_fwd_gn (32 groups) on every 3x3 stride-1 / Upsample row and the general kernel's, and the concatenated
    input / split output of the 1x1 rows, S = 1 .. 368 over the channels they are legal for."""
    shape, s, ci, co = _points()
    S, Ci, Co = cp._grid()
    for H, W, KS, mode in cp.rows():
        if mode in (0, 2):
            ok = co % cp.GROUPS == 0
            d = cp.plan_arrays(S, Ci, Co, H, W, KS, mode, gn=cp.GROUPS)
            need = np.broadcast_to(d["need"], shape).ravel()
            got = _query(lib, s[ok], ci[ok], co[ok], H, W, KS, mode, 0, 0, cp.GROUPS, 1, need[ok])
            want = _want(d, shape)[ok]
            bad = np.nonzero((got != want).any(1))[0]
            assert bad.size == 0, ((H, W, KS, mode, "gn"), int(s[ok][bad[0]]), int(ci[ok][bad[0]]), int(co[ok][bad[0]]),
                                   got[bad[0]].tolist(), want[bad[0]].tolist())
        if KS == 1:
            for C1 in (32, 64, 192):
                ok = (ci > C1) & (ci % 1 == 0)
                d = cp.plan_arrays(S, Ci, Co, H, W, KS, mode, C1=C1)
                need = np.broadcast_to(d["need"], shape).ravel()
                got = _query(lib, s[ok], ci[ok], co[ok], H, W, KS, mode, C1, 0, 0, 1, need[ok])
                assert np.array_equal(got, _want(d, shape)[ok]), (H, W, "cat", C1)
            for C1o in (64, 192):
                ok = co > C1o
                d = cp.plan_arrays(S, Ci, Co, H, W, KS, mode, C1o=C1o)
                need = np.broadcast_to(d["need"], shape).ravel()
                got = _query(lib, s[ok], ci[ok], co[ok], H, W, KS, mode, 0, C1o, 0, 1, need[ok])
                assert np.array_equal(got, _want(d, shape)[ok]) and np.all(got[:, 3] == 1), (H, W, "split output", C1o)


def test_the_query_refuses_what_the_entries_refuse(lib):
    out = (ctypes.c_int * 8)()
    p = ctypes.cast(out, ctypes.c_void_p)
    q = lambda *a: lib.vf_conv_fwd_plan(*a, p)
    assert q(2, 64, 64, 16, 16, 3, 0, 0, 0, 0, 1, 0) == 0 and list(out)[:4] == [0, 1, 8, 1]
    for bad in ((2, 64, 64, 16, 16, 5, 0, 0, 0, 0, 0, 0), (2, 64, 64, 16, 16, 1, 1, 0, 0, 0, 0, 0), (2, 64, 64, 16, 16, 3, 3, 0, 0, 0, 0, 0),
                (2, 64, 64, 16, 16, 3, 0, 32, 0, 0, 0, 0), (2, 64, 64, 16, 16, 1, 0, 16, 0, 0, 0, 0), (2, 64, 128, 16, 16, 1, 0, 0, 32, 0, 0, 0),
                (2, 64, 96, 16, 16, 3, 0, 0, 0, 64, 0, 0), (2, 64, 64, 16, 16, 3, 4, 0, 0, 32, 0, 0), (2, 64, 128, 16, 16, 1, 0, 0, 64, 32, 0, 0),
                (0, 64, 64, 16, 16, 3, 0, 0, 0, 0, 0, 0), (2, 64, 64, 5, 5, 3, 2, 0, 0, 0, 0, 0)):
        assert q(*bad) == 1, bad
    assert lib.vf_conv_fwd_plan(2, 64, 64, 16, 16, 3, 0, 0, 0, 0, 0, 0, None) == 1


def test_mode_4_ignores_the_workspace(lib):
    """The sub-pixel dgrad's epilogue has no partial-sum form: whatever workspace is passed, one K range."""
    shape, s, ci, co = _points()
    for W in cp.SPEC_MAPS[3, 4]:
        got = _query(lib, s, ci, co, W, W, 3, 4, 0, 0, 0, 1, 1 << 40)
        assert np.all(got[:, 3] == 1) and np.all(got[:, 5] == cp.RED_NONE), W
    c = cp.SPECIALS[0]
    assert c.mode == 4 and cp.plan(c)["ks0"] == 16 and cp.plan(c)["ks"] == 1 and cp.plan(c)["need"] == 16 * c.S * c.Cout * c.H * c.W


def test_every_class_the_models_reach_is_in_the_case_list():
    reached, have = cp.covered_classes(), cp.case_classes()
    print()
    for k in sorted(set(reached) | have, key=str):
        print(f"CLASS | {' | '.join(str(v) for v in k)} | first reached at {reached.get(k, 'not by the models')} | "
              f"{'in cases()' if k in have else 'NOT COVERED'}")
    fam = lambda ks: dict(sorted({f: sum(k[0] == f for k in ks) for f in {k[0] for k in ks}}.items()))
    print(f"reached classes {len(reached)} {fam(reached)}; classes in cases() {len(have)} {fam(have)}; cases {len(cp.cases())}")
    assert {"tile", "split", "pad", "safe", "any", "cat", "split output", "reduce plain", "reduce+gn", "gn fallback", "1x1 kernel",
            "mode 4 with a priced workspace"} <= {k[0] for k in reached} | {k[0] for k in have}
    over = cp.over_cap_classes()
    for k, (c, macs) in sorted(over.items(), key=lambda kv: str(kv[0])):
        print(f"OVER THE CAP | {' | '.join(str(v) for v in k)} | cheapest {cp.case_id(c)} at {macs:.2e} multiply-adds")
    assert not set(over) & have and all(macs > cp.CAP_MACS for _, macs in over.values())
    # (every such class needs conv1x1_kernel<2>'s own grid: Cin >= 224, 512 column tiles of 128 pixels x 128 channels)
    assert all(cp.ROUTES[cp.ONE128] in k or "<2>" in str(k) for k in over), sorted(over, key=str)
    assert set(reached) <= have | set(over), sorted(set(reached) - have - set(over), key=str)


def test_case_list_is_deterministic_capped_and_holds_the_named_cases():
    cs = cp.cases()
    cp._enumerate.cache_clear()
    assert cp.cases() == cs and len({cp.case_id(c) for c in cs}) == len(cs)
    D = [(c, cp.plan(c)) for c in cs]
    for c, d in D:
        assert cp.cost(c) <= cp.CAP_MACS, (cp.case_id(c), cp.cost(c), c.why)
        assert (d["route"] == cp.ANY) == (not cp.fwd_specialised(c.KS, c.H, c.W, c.mode))
        assert not c.C1 or (c.KS == 1 and c.C1 % 32 == 0 and 0 < c.C1 < c.Cin)
        assert not c.C1o or (c.KS == 1 and c.C1o % 64 == 0 and 0 < c.C1o < c.Cout)
        assert not c.gn or (c.Cout % c.gn == 0 and c.mode != 4 and not c.C1 and not c.C1o)
    keys = cp.case_classes()
    # the issue's list: a 16-way split, a partly filled second batch, an uneven range, a half-empty 8x8 tile under a split,
    # every pricing state, all six reduce + GroupNorm variants with and without clamped lanes, both fallbacks, both
    # 1x1 kernels on either side of every threshold, the general kernel's branches
    assert {k[3] for k in keys if k[0] == "split"} == set(cp.KSB) and {k[5] for k in keys if k[0] == "split"} == set(cp.PRICING)
    assert any(k[0] == "split" and k[4] == "uneven" and k[3] != "1" for k in keys)
    # a half-empty 8x8 tile (two views per 128-pixel tile, odd S) never meets a split: 128-pixel tiles are taken from 768
    # workgroups on, a split below 256 -- so the SAFE predicate's S % IM term and the split do not interact
    assert any(k[0] == "tile" and k[6] == "half-empty last tile" for k in keys)
    S, Ci, Co = cp._grid()
    for (KS, mode), maps in cp.SPEC_MAPS.items():
        d = cp.plan_arrays(S, Ci, Co, maps[0], maps[0], KS, mode)
        assert not np.any(d["half"] & (d["ks0"] > 1)) and bool(np.any(d["half"])) == (maps[0] == 8)
    assert {(k[1], k[2]) for k in keys if k[0] == "reduce+gn"} == {(v, t) for _, v, t in cp.GN_TABLE}
    assert {k[3] for k in keys if k[0] == "reduce+gn"} == {"fills", "clamped lanes"}
    assert {k[4] for k in keys if k[0] == "reduce+gn"} == {"whole batches", "partly filled batch"}
    assert {k[5] for k in keys if k[0] == "reduce+gn"} == {"store_y", "no y"}
    assert {k[1] for k in keys if k[0] == "gn fallback"} == {"gn launch", "plain, gn launch"}
    # (conv1x1_kernel<2>'s own thresholds lie above the cap: over_cap_classes names them)
    assert {k[2] for k in keys if k[0] == "1x1 route"} == set(cp.ONE_EDGES[6:])
    assert {k[2] for k in cp.over_cap_classes() if k[0] == "1x1 route"} == set(cp.ONE_EDGES[:6])
    assert {k[1] for k in keys if k[0] == "1x1 kernel"} == {cp.ROUTES[cp.ONE64]}
    assert {k[2] for k in keys if k[0] == "cat"} == {"unsplit", "on a split boundary", "inside a split"}
    assert any(k[0] == "cat" and k[3] == "second part % 32" for k in keys)
    assert {k[1] for k in keys if k[0] == "split output"} >= {"conv_mfma", "conv_any"}
    assert {k[1:3] for k in keys if k[0] == "safe"} >= {("SAFE", ""), ("guarded", "Cin % 32"), ("guarded", "")}
    assert {k[2:4] for k in keys if k[0] == "reduce plain"} == {(a, b) for a in ("whole", "ragged") for b in ("one batch", "second batch")}
    assert {(c.H, c.W, c.KS, c.mode) for c, d in D if d["route"] == cp.ANY} == set(cp.ANY_SHAPES)
    assert {"mode 4 with a priced workspace"} <= {k[0] for k in keys}
    assert any(c.mode == 4 and d["route"] == cp.MFMA and d["ks0"] > 1 and d["need"] > 0 for c, d in D)
    assert any((c.S, c.Cout, c.W, c.gn) == (22, 192, 16, g) for c, _ in D for g in (0, 32))
    assert any((c.S, c.Cout, c.W, c.gn) == (1, 64, 128, 32) and (d["nv"], d["nt"]) == (8, 1024) for c, d in D)
    assert any(c.gn and c.Cout // c.gn == 3 for c, _ in D) and any(c.gn and c.Cout // c.gn == 10 for c, _ in D)
    assert len(cp.hygiene_cases()) >= 12 and len(cp.clip_cases()) >= 4


def test_chunk_ranges_tile_k():
    for nch in range(1, 130):
        for ks in range(1, min(nch, 16) + 1):
            r = cp.chunk_ranges(nch, ks)
            assert r[0][0] == 0 and r[-1][1] == nch and all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(e > b for b, e in r)


# ---------------------------------------------------------------------------------------- the inputs discriminate
@pytest.mark.parametrize("part", range(4))
def test_split_model_passes_the_rule_and_every_mutant_fails_it(part):
    """For every case with a split, a concatenation, a half-empty tile or clamped GroupNorm lanes: the decomposition
    evaluated in fp32 on the CPU PASSES the rule of the GPU tests at tol = 2e-5, and each applicable wrong decomposition
    (conv_plan_ref.MUTANTS) FAILS it."""
    n, seen = 0, set()
    print()
    for c in cp.cases()[part::4]:
        d = cp.plan(c)
        ms = [m for m in cp.MUTANTS if cp.mutant_applies(c, d, m)]
        if not ms:
            continue
        t = cp.inputs(c)
        r64, r32 = cp.conv_ref(t, c, torch.float64), cp.conv_ref(t, c, torch.float32)
        got = cp.conv_split(t, c, d)
        for a, b64, b32 in zip(got, r64, r32):
            err, e, bound, ok = cr.judge(a, b64, b32, cp.TOL)
            assert ok, (cp.case_id(c), err, bound)
        line = [f"MUTANT | {cp.case_id(c)} | ks {d['ks']} | split model {cr.err(got[0], r64[0]):.1e}"]
        for m in ms:
            bad = cp.conv_split(t, c, d, mutate=m)
            k = 1 if m == "gn_clamped_lanes" else 0
            err, e, bound, ok = cr.judge(bad[k], r64[k], r32[k], cp.TOL)
            line.append(f"{m} {err:.1e}")
            assert not ok, (cp.case_id(c), m, err, bound)
            n += 1
            seen.add(m)
        print(" | ".join(line))
    assert n >= 10, (n, seen)


def test_every_mutant_has_cases_it_applies_to():
    D = [(c, cp.plan(c)) for c in cp.cases()]
    for m in cp.MUTANTS:
        assert sum(cp.mutant_applies(c, d, m) for c, d in D) >= 2, m


def test_knobs_fail_loudly():
    """(On a copy of the environment: the library reads each variable once per process, so no test may set it.)"""
    for k in cp.ENV:
        with pytest.raises(RuntimeError, match=k):
            cp.check_env({k: "1"})
    assert len(cp.ENV) == 6
    cp.check_env({})
    cp.check_env()
