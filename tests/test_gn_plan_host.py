"""The GroupNorm launch plans on the CPU: tests/gn_plan_ref.py's restatement equals the host functions of libvf_hip.so
(all twelve fields of vf_gn_plan, and vf_gn_bwd_emits_rowsum) over the whole domain, every plan class the SMALL / TINY
networks' GroupNorm layers reach is in gn_plan_ref.cases() -- the list tests/test_gpu_gn_plan.py runs -- every case stays
under the float limit with a reference error below cond_ref.CAP, and the comparison rule of those tests accepts a CPU fp32
model of the kernels and rejects seven wrong ones on the inputs they use.

vf_gn_plan is the function the launchers execute (csrc/norm.hip: vf_gn_cat_fwd / vf_gn_cat_bwd run gn_plan and launch what
it says), so pinning it pins the launch.

The sweep (the plan is a function of (C, HW, groups, cat, C1, has_addend, has_addend2, has_dx2); one library call per point):
  * every (C, groups) with C = 1 .. 1024 (and the larger C of the case list) and groups a divisor of C, at every power-of-
    two HW from 1 to 65536: plain with all eight addend / dx2 states; concatenated at C1 = 1, C / 2, C - 1 with all eight
    states, and at C1 = 0, C, -1 with everything passed;
  * every HW from 1 to 4096 at every C = 1 .. 1024 with the largest divisor of C that is at most 32 as groups: plain with
    nothing passed, concatenated at C1 = C / 2 with everything passed (off the powers of two the answer does not look at
    the optional pointers: the first sweep pins that at HW = 1 and 2, this one at every other HW for these two states);
  * groups that do not divide C, zero and negative groups, HW <= 0.
The full product of the issue's axes (C x HW x divisors x 40 states, 1.2e9 points) is out of reach of one ctypes call
per point; the two sweeps cross every axis with the ones it can interact with (1.3e7 points)."""
import concurrent.futures
import ctypes
import itertools
import multiprocessing
import os

import numpy as np
import pytest
import torch

import cond_ref as cr
import gn_plan_ref as gp

POW2 = tuple(1 << k for k in range(17))
STATES = tuple(itertools.product((0, 1), repeat=3))       # (has_addend, has_addend2, has_dx2)


@pytest.fixture(scope="module")
def lib():
    from view_fusion_amd import _lib
    return _lib.load()


def _query(lib, C, HW, groups, cat, C1, a1, a2, dx2):
    """vf_gn_plan at every point (arrays broadcast together) -> (n, 12) int32."""
    args = [np.ascontiguousarray(a).ravel() for a in np.broadcast_arrays(C, HW, groups, cat, C1, a1, a2, dx2)]
    n = args[0].size
    out = np.full((n, 12), -1, dtype=np.int32)
    base = out.ctypes.data
    rcs = list(map(lib.vf_gn_plan, *(a.tolist() for a in args), range(base, base + 48 * n, 48)))
    assert not any(rcs)
    return out, args


def _compare(lib, label, C, HW, groups, cat, C1, a1, a2, dx2):
    got, args = _query(lib, C, HW, groups, cat, C1, a1, a2, dx2)
    d = gp.plan_arrays(*args)
    want = np.stack([d[k] for k in gp.FIELDS], 1)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (label, dict(zip(("C", "HW", "groups", "cat", "C1", "addend", "addend2", "dx2"), (int(a[bad[0]]) for a in args))),
                           dict(zip(gp.FIELDS, got[bad[0]].tolist())), dict(zip(gp.FIELDS, want[bad[0]].tolist())))
    return got.shape[0]


def _pairs():
    """(C, groups) with groups | C: C = 1 .. 1024 and the larger C of the case list."""
    cs = sorted(set(range(1, 1025)) | {c.C for c in gp.cases()})
    return np.array([(C, g) for C in cs for g in range(1, min(C, 1024) + 1) if C % g == 0] +
                    [(C, C) for C in cs if C > 1024], dtype=np.int64)


def _check_pow2(HW):
    """One power-of-two HW of the first sweep -> points checked (a top-level function: the rows run in worker processes,
    the library's host functions being pure)."""
    from view_fusion_amd import _lib
    lib = _lib.load()
    pg = _pairs()
    C, g = pg[:, 0][:, None], pg[:, 1][:, None]
    st = np.array(STATES, dtype=np.int64)
    a1, a2, dx2 = st[None, :, 0], st[None, :, 1], st[None, :, 2]
    n = _compare(lib, ("plain", HW), C, HW, g, 0, C, a1, a2, dx2)
    for name, C1 in (("1", 1 + 0 * C), ("C / 2", C // 2), ("C - 1", C - 1)):
        n += _compare(lib, ("cat", name, HW), C, HW, g, 1, C1, a1, a2, dx2)
    for name, C1 in (("0", 0 * C), ("C", C), ("-1", 0 * C - 1)):
        n += _compare(lib, ("cat", name, HW), C, HW, g, 1, C1, 1, 1, 1)
    got = np.array(list(map(lib.vf_gn_bwd_emits_rowsum, pg[:, 0].tolist(), itertools.repeat(HW), pg[:, 1].tolist())))
    assert np.array_equal(got, gp.emits_rowsum(pg[:, 0], HW, pg[:, 1])), HW
    return n


def _check_hw_block(lo):
    from view_fusion_amd import _lib
    lib = _lib.load()
    C = np.arange(1, 1025, dtype=np.int64)[:, None]
    g = np.array([max(k for k in range(1, 33) if c % k == 0) for c in range(1, 1025)], dtype=np.int64)[:, None]
    HW = np.arange(lo, min(lo + 256, 4097), dtype=np.int64)[None, :]
    n = _compare(lib, ("every HW, plain", lo), C, HW, g, 0, C, 0, 0, 0)
    n += _compare(lib, ("every HW, cat", lo), C, HW, g, 1, C // 2, 1, 1, 1)
    Cf, HWf, gf = (a.ravel() for a in np.broadcast_arrays(C, HW, g))
    got = np.array(list(map(lib.vf_gn_bwd_emits_rowsum, Cf.tolist(), HWf.tolist(), gf.tolist())))
    assert np.array_equal(got, gp.emits_rowsum(Cf, HWf, gf)), lo
    return n


def test_the_plan_equals_the_library_on_the_whole_sweep(lib):
    jobs = [(_check_pow2, HW) for HW in POW2] + [(_check_hw_block, lo) for lo in range(1, 4097, 256)]
    workers = min(8, len(os.sched_getaffinity(0)))
    if workers > 1:
        with concurrent.futures.ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as pool:
            n = sum(f.result() for f in [pool.submit(fn, a) for fn, a in jobs])
    else:
        n = sum(fn(a) for fn, a in jobs)
    print(f"\n{n} points")
    assert n == len(POW2) * len(_pairs()) * (8 + 24 + 3) + 2 * 1024 * 4096


def test_refusals_and_degenerate_arguments(lib):
    """Groups that do not divide C, zero / negative groups, HW <= 0, a NULL out; every named refusal of the issue."""
    C = np.arange(1, 65, dtype=np.int64)[:, None, None]
    g = np.arange(-2, 70, dtype=np.int64)[None, :, None]
    HW = np.array([-4, 0, 1, 3, 4, 60, 64, 256], dtype=np.int64)[None, None, :]
    for cat, C1 in ((0, C), (1, np.maximum(C // 2, 1))):
        _compare(lib, ("any groups", cat), C, HW, g, cat, C1, 1, 1, 1)
    assert lib.vf_gn_plan(64, 64, 32, 0, 64, 0, 0, 0, None) == 1
    out = (ctypes.c_int * 12)()
    seen = set()
    for args, which, why in gp.REJECTIONS:
        assert lib.vf_gn_plan(*args, ctypes.cast(out, ctypes.c_void_p)) == 0
        d = dict(zip(gp.FIELDS, out))
        assert d["bwd"] == gp.REJECTED and (d["fwd"] == gp.REJECTED) == (which == "both"), (args, why, d)
        assert [d[k] for k in gp.FIELDS[:-1] if k not in ("fwd", "fnv", "fnt")] == [0] * 8, (args, d)
        seen.add(why)
    assert seen == {"groups <= 0", "C % groups != 0", "cat with HW not a power of two", "cat with HW < 4", "C1 <= 0", "C1 >= C",
                    "cat where the fused backward does not apply", "cat with addend but no addend2", "cat without dx2"}
    for C, HW, groups in ((64, 64, 0), (64, 64, 5), (64, 60, 32), (64, 2, 32), (64, 0, 32)):
        assert lib.vf_gn_bwd_emits_rowsum(C, HW, groups) == 0


def test_every_class_the_models_reach_is_in_the_case_list():
    layers = gp.model_layers()
    assert len(layers) >= 30 and any(c1 for *_, c1 in layers) and {h for _, h, _, _ in layers} == {8, 16, 32, 64}
    covered = {k for c in gp.cases() for k in gp.plan_class(c.C, c.H * c.W, c.groups, c.C1)}
    reached = {}
    for C, H, g, C1 in layers:
        for k in gp.plan_class(C, H * H, g, C1):
            reached.setdefault(k, (C, H, g, C1))
    print()
    for k in sorted(set(reached) | covered, key=str):
        print(f"CLASS | {' | '.join(str(v) for v in k)} | first reached at {reached.get(k, 'not by the models')} | "
              f"{'in cases()' if k in covered else 'NOT COVERED'}")
    assert {"fwd shift", "fwd input", "cat", "bwd", "bwd input"} <= {k[0] for k in reached}
    assert any(k[0] == "cat" and k[1] == "inside a group" for k in reached), "the decoder's 64-aligned splits fall inside groups"
    assert set(reached) <= covered, sorted(set(reached) - covered, key=str)


def test_case_list_is_deterministic_capped_and_holds_every_required_key():
    cs = gp.cases()
    gp._enumerate.cache_clear()
    assert gp.cases() == cs and len({gp.case_id(c) for c in cs}) == len(cs)
    have, req = gp.case_classes(), gp.required_keys()
    assert not gp.over_cap_classes() and req <= have, sorted(req - have, key=str)
    for c in cs:
        d = gp.plan(c)
        assert gp.floats(c) <= gp.MAX_FLOATS and c.S in (1, 2, 3) and c.groups in gp.GROUPS_DOMAIN, gp.case_id(c)
        assert d["cpg"] * c.H * c.W >= 3, "groups of one or two elements are outside the domain"
        assert (c.S >= 2 and c.groups >= 2) or "one view, one group" in c.why
        assert d["fwd"] != gp.REJECTED and (d["bwd"] != gp.REJECTED or c.C1)
    # the issue's list, spelled out
    assert {(k[1], k[2]) for k in have if k[0] == "fwd"} == {(v, t) for _, v, t in gp.FWD_TABLE}
    assert {k[1:4] for k in have if k[0] == "bwd" and k[1] == 16} == {(16, v, t) for _, v, t in gp.BWD16_TABLE}
    assert {k[1:4] for k in have if k[0] == "bwd" and k[1] == 64} == {(64, v, t) for _, v, t in gp.BWD64_TABLE}
    assert ("fwd", 2, 256, "empty slot") not in req and sum(k[0] == "fwd" and k[3] == "empty slot" for k in req) == 8
    assert {k[1] for k in have if k[0] == "bwd two chunks"} == {"1", "2", "> 2"}
    assert any(gp.plan(c)["bwd"] == gp.BWD_TWO and gp.plan(c)["chunks"] > 1 for c in cs), "chunks > 1 with addends (every state runs)"
    assert any(c.groups == 32 and gp.plan(c)["bwd"] == gp.BWD_TWO for c in cs) and any(c.groups == 3 and c.C1 for c in cs)


_REFS = {}


def _refs(c, silu):
    key = (c[:-2], silu)
    if key not in _REFS:
        if len(_REFS) > 4:
            _REFS.clear()
        t = gp.inputs(c)
        _REFS[key] = (t, *gp.refs(c, t, silu))
    return _REFS[key]


def _states(c):
    return ("none", "both") if c.C1 else gp.ADDEND_STATES


@pytest.mark.parametrize("part", range(8))
def test_the_rule_accepts_the_kernel_model_and_rejects_seven_wrong_ones(part):
    """On every case: cond_ref.bound accepts the stock fp32 error e of every output (e <= CAP), the CPU fp32 model of the
    kernels passes cond_ref.judge on every output and addend state, and every wrong model fails it on every case it applies
    to (gn_plan_ref.mutant_applies states which); a wrong model that applies to no case is an error of the case list."""
    cs = gp.cases()[part::8]
    applied = {m: 0 for m in gp.MUTANTS}
    print()
    for c in cs:
        d = gp.plan(c)
        t, r64, r32 = _refs(c, c.silu)
        if c.C1:
            t = gp.cat_addend(t, c)
        for state in _states(c):
            a64, a32 = gp.with_addends(r64, t, state, torch.float64), gp.with_addends(r32, t, state, torch.float32)
            rows = gp.judge_all(gp.kernel_model(c, t, c.silu, state), a64, a32)
            assert all(r[2] <= cr.CAP for r in rows)
            assert all(r[4] for r in rows), (gp.case_id(c), state, [r for r in rows if not r[4]])
            if state == _states(c)[-1]:
                print(f"GNPLAN-HOST | {gp.case_id(c)} | " + " ".join(f"{r[0]} e {r[2]:.1e} err {r[1]:.1e}" for r in rows))
            for m in gp.MUTANTS:
                if state != _states(c)[-1] and m != "drop_addend2":
                    continue                             # (the addend state does not interact with the other six)
                if gp.mutant_applies(c, d, m, state):
                    applied[m] += 1
                    rows = gp.judge_all(gp.kernel_model(c, t, c.silu, state, m), a64, a32)
                    assert not all(r[4] for r in rows), (gp.case_id(c), state, m, "passes the rule")
    assert all(applied.values()), applied
