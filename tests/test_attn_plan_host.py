"""The attention / batched-GEMM / softmax launch plans on the CPU: tests/attn_plan_ref.py's restatement equals the host
functions of libvf_hip.so (vf_attention_fwd_kernel, vf_attention_bwd_plan, vf_bgemm_plan, vf_softmax_plan) on the sweep
S = 1 .. 400 x C in {32, 48, 64, 96, ..., 512} x L in {25, 60, 64, 81, 144, 256, 1024, 1296, 4096, 4097}, for every product of
ops.attention / ops.linear at those shapes and on raw stride tuples that flip each term of the fast predicate alone; the
Python route of ops/attention.py and the launch list tests/test_gpu_conditioning.py expects agree with the plans; the three
block-id maps are bijections that keep the tiles of an item on one XCD, and four wrong variants are not; every class the
SMALL / TINY networks reach at S = 1 .. 368 is in the case lists tests/test_gpu_attn_plan.py runs.

The planners are the functions the launchers execute (vf_bgemm runs bgemm_plan, the softmax launchers softmax_maxv,
vf_attention_dscore / _dvdk the predicates and grids vf_attention_bwd_plan reports), so pinning them pins the launch."""
import ctypes
import itertools

import pytest

import attn_plan_ref as ap
import cond_ref as cr


@pytest.fixture(scope="module")
def lib():
    from view_fusion_amd import _lib
    return _lib.load()


def _ints(n):
    buf = (ctypes.c_int * n)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _lib_bgemm_plan(lib, alignA, alignB, batch, M, N, K, sA, sB, sCn):
    buf, p = _ints(7)
    assert lib.vf_bgemm_plan(ctypes.c_void_p(4096 + alignA), ctypes.c_void_p(4096 + alignB), batch, M, N, K, *sA, *sB, sCn, p) == 0
    return list(buf)


def test_the_attention_plans_equal_the_library_on_the_whole_sweep(lib):
    buf, p = _ints(6)
    n = 0
    for S, C, L in itertools.product(ap.SWEEP_S, ap.SWEEP_C, ap.SWEEP_L):
        assert lib.vf_attention_fwd_kernel(S, C, L) == ap.fwd_kernel(S, C, L), (S, C, L)
        for ds, dv in ((1, 1), (1, 0), (0, 1), (0, 0)):
            assert lib.vf_attention_bwd_plan(S, C, L, ds, dv, p) == 0
            assert list(buf) == ap.bwd_plan(S, C, L, ds, dv), (S, C, L, ds, dv, list(buf))
            n += 1
    for S, C, L in ((0, 64, 256), (-1, 64, 256), (4, 0, 256), (4, 64, 0), (4, -32, 64)):
        assert lib.vf_attention_fwd_kernel(S, C, L) == ap.fwd_kernel(S, C, L) == 0
        assert lib.vf_attention_bwd_plan(S, C, L, 1, 1, p) == 0 and list(buf) == ap.bwd_plan(S, C, L) == [0] * 6
    assert lib.vf_attention_bwd_plan(4, 64, 256, 1, 1, None) == 1
    print(f"\n{n} backward plans")
    # the issue's statement of the forward rule, spelled out
    to_kh = [S for S in range(17, 401) if ap.fwd_kernel(S, 32, 256) == ap.KH]
    assert to_kh == list(range(97, 129)) + list(range(225, 257)) + list(range(353, 385))
    assert all(ap.fwd_kernel(S, 64, L) == ap.Q16 and ap.fwd_kernel(S, 96, L) != ap.Q16 for S in range(1, 17) for L in (64, 256))
    assert ap.fwd_kernel(17, 64, 64) == ap.SPLIT == ap.fwd_kernel(3, 96, 64) and ap.fwd_kernel(3, 64, 256, q32=False, q16=False) == ap.SPLIT
    assert ap.fwd_kernel(52, 32, 256, q32=False) == ap.SPLIT and ap.fwd_kernel(53, 32, 256, q32=False) == ap.KH


def test_the_python_route_and_the_expected_launch_lists_agree_with_the_plans(lib, monkeypatch):
    from view_fusion_amd import ops
    import test_gpu_conditioning as tc
    for ds, dv in ((1, 1), (1, 0), (0, 1), (0, 0)):
        monkeypatch.setattr(ops.st, "ATTN_DSCORE", bool(ds))
        monkeypatch.setattr(ops.st, "ATTN_DVDK", bool(dv))
        for C, L in itertools.product(ap.SWEEP_C, ap.SWEEP_L):
            plan = ap.bwd_plan(3, C, L, ds, dv)
            route = ops.attention_route(C, L)
            assert (route == "stream") == (plan[0] == ap.BWD_NONE) == (L > 4096), (C, L)
            if route == "stream":
                continue
            assert (route == "fused") == (ap.fwd_launches(C, L) == ["vf_attention_fwd"]), (C, L)
            assert (route == "fused") == (L in (64, 256) and ap.fwd_kernel(3, C, L) != ap.REFUSED)
            assert ops.attention_bwd_route(C, L) == (plan[0] in (1, 2), plan[0] == 1), (C, L, ds, dv)
            if ds and dv:
                assert tc._attn_launches(C, L) == ap.fwd_launches(C, L) + ap.bwd_launches(plan), (C, L)
    for key, name in tc.ATTN_KERNEL.items():
        C, H, W, S = key
        assert ap.fwd_key(S, C, H * W)[1] == name, key


def test_the_bgemm_plan_equals_the_library_for_every_product_and_each_predicate_term(lib):
    n, seen = 0, {}
    for S, C, L in itertools.product(ap.SWEEP_S, ap.SWEEP_C, ap.SWEEP_L[:-1]):
        for pr in ap.attention_products(S, C, L):
            got = _lib_bgemm_plan(lib, 4 * pr.offA, 4 * pr.offB, pr.batch, pr.M, pr.N, pr.K, pr.sA[:3], pr.sB[:3], pr.sC[2])
            assert got == ap.product_plan(pr), (S, C, L, pr.name, got)
            seen.setdefault((pr.name, ap.VARIANT_NAMES[got[1]]), (S, C, L))
            n += 1
    for S, I, O in itertools.product(ap.SWEEP_S, (32, 64, 128, 256), (32, 64, 128, 256)):
        for pr in ap.linear_products(S, I, O):
            got = _lib_bgemm_plan(lib, 0, 0, pr.batch, pr.M, pr.N, pr.K, pr.sA, pr.sB, pr.sC[2])
            assert got == ap.product_plan(pr), (S, I, O, pr.name, got)
            seen.setdefault((pr.name, ap.VARIANT_NAMES[got[1]]), (S, I, O))
            n += 1
    print(f"\n{n} product plans")
    for k, v in sorted(seen.items()):
        print(f"PRODUCT | {k[0]} | {k[1]} | first at {v}")
    # which kernel each product takes: the fast one wherever L (and for dw, S) is a multiple of four
    assert {k for k in seen if k[1] != "slow"} == {("qk", "FF"), ("pv", "TT"), ("dp", "FF"), ("dv", "TF"), ("dq", "TT"), ("dk", "TF"),
                                                   ("lin", "TT"), ("lin dx", "TF"), ("lin dw", "FF")}
    assert not any(k[1] == "FT" for k in seen), "no product of ops reaches bgemm_v2_kernel<false, true>: direct cases only"
    assert all((n_, "slow") in seen for n_ in ("qk", "pv", "dp", "dv", "dq", "dk", "lin dw"))
    # raw stride tuples: from a point that passes, each term flipped alone
    base = dict(aA=0, aB=0, batch=3, M=8, N=8, K=8, sA=[64, 8, 1], sB=[64, 8, 1], sCn=1)
    flips = [("A no unit stride", dict(sA=[64, 8, 4])), ("B no unit stride", dict(sB=[256, 32, 4])), ("sCn != 1", dict(sCn=3)),
             ("K % 4", dict(K=6)), ("sAb % 4", dict(sA=[65, 8, 1])), ("sBb % 4", dict(sB=[66, 8, 1])),
             ("sAm % 4", dict(sA=[64, 9, 1])), ("sAk % 4", dict(sA=[64, 1, 10])), ("M % 4", dict(M=7, sA=[64, 1, 8])),
             ("sBn % 4", dict(sB=[64, 1, 9])), ("sBk % 4", dict(sB=[64, 10, 1])), ("N % 4", dict(N=5)),
             ("A | B not 16-byte aligned", dict(aA=4)), ("A | B not 16-byte aligned", dict(aB=8))]
    for a, b in itertools.product((1, 8), repeat=2):       # the four variants from the same point
        d = dict(base, sA=[64, a, 9 - a], sB=[64, b, 9 - b])
        got = _lib_bgemm_plan(lib, 0, 0, d["batch"], d["M"], d["N"], d["K"], d["sA"], d["sB"], 1)
        assert got == ap.bgemm_plan(0, 0, 3, 8, 8, 8, *d["sA"], *d["sB"], 1) and got[6] == 0
        assert got[1] == {(8, 8): ap.TF, (8, 1): ap.TT, (1, 8): ap.FF, (1, 1): ap.FT}[(a, b)]
    for name, change in flips:
        d = dict(base, **change)
        got = _lib_bgemm_plan(lib, d["aA"], d["aB"], d["batch"], d["M"], d["N"], d["K"], d["sA"], d["sB"], d["sCn"])
        assert got == ap.bgemm_plan(d["aA"], d["aB"], d["batch"], d["M"], d["N"], d["K"], *d["sA"], *d["sB"], d["sCn"]), name
        assert got[1] == ap.SLOW and ap.refusal_names(got[6]) == (name,), (name, ap.refusal_names(got[6]))
    assert {n_ for n_, _ in flips} == set(ap.REFUSAL_BITS)
    for batch, M, N in ((0, 8, 8), (3, 0, 8), (3, 8, -1)):
        assert _lib_bgemm_plan(lib, 0, 0, batch, M, N, 8, [64, 8, 1], [64, 8, 1], 1) == [0] * 7
    for batch in (1, 7, 8, 9, 400):
        assert _lib_bgemm_plan(lib, 0, 0, batch, 70, 130, 8, [1024, 8, 1], [2048, 136, 1], 1)[2:6] == [3, 2, batch, batch // 8]
    assert lib.vf_bgemm_plan(None, None, 1, 8, 8, 8, 64, 8, 1, 64, 8, 1, 1, None) == 1


def test_the_softmax_plan_equals_the_library(lib):
    buf, p = _ints(2)
    for rows, cols in itertools.product((-1, 0, 1, 3, 4, 5, 1000), list(range(-1, 4200)) + [1 << 20]):
        assert lib.vf_softmax_plan(rows, cols, p) == 0 and list(buf) == ap.softmax_plan(rows, cols), (rows, cols)
    assert [ap.softmax_maxv(c) for c in (64, 65, 256, 257, 1024, 1025, 4096, 4097)] == [1, 4, 4, 16, 16, 64, 64, 0]
    assert lib.vf_softmax_plan(4, 64, None) == 1


def test_the_three_block_id_maps_are_bijections_that_keep_an_item_on_one_xcd():
    """attn_fwd_q32_kernel (S = 1 .. 400), attn_bwd_dvdk_kernel and bgemm_v2_kernel (S / batch = 1 .. 400 at nt in {1, 2,
    4, 12, 16}): every work item exactly once, and the tiles of an item of a whole group of eight in consecutive slots of
    one XCD (blocks i, i + 8, ... share an XCD)."""
    for n in range(1, 401):
        assert ap.map_faults("q32", n, 8) == [], n
        for nt in (1, 2, 4, 12, 16):
            assert ap.map_faults("dvdk", n, nt) == [], (n, nt)
            assert ap.map_faults("bgemm", n, nt) == [], (n, nt)
    # a two-dimensional grid takes the same map: tile = by gx + bx
    for gx, gy, batch in ((3, 2, 11), (1, 5, 8), (4, 4, 17)):
        items = [ap.bgemm_map(i, gx, gy, batch, batch // 8) for i in range(gx * gy * batch)]
        assert sorted(items) == [(b, t) for b in range(batch) for t in range(gx * gy)]


@pytest.mark.parametrize("mutant", sorted(ap.MUTANTS))
def test_a_wrong_map_is_not_a_bijection(mutant):
    """Each wrong variant breaks the bijection, and shows where: the 32-query remainder only at S = 8 g + r, the others from
    the first whole group on -- the sizes the case lists therefore hold."""
    which = ap.MUTANTS[mutant]
    nts = (8,) if which == "q32" else (1, 2, 4, 12, 16)
    bad = sorted({n for n in range(1, 401) for nt in nts if ap.map_faults(which, n, nt, mutant)})
    print(f"\nMUTANT | {mutant} | {which} | wrong at {len(bad)} of 400 sizes, first {bad[:6]}")
    assert bad
    if mutant == "remainder base shifted wrongly":
        assert bad == [n for n in range(9, 401) if n % 8], "caught exactly where a remainder follows a whole group"
        out = ap.permuted_views(11, mutant)
        assert out is not None and (out[8:] == -1).all(), "views 8 .. 10 are never written, views 4 .. 6 twice"
        assert (ap.permuted_views(11, None) >= 0).all()
    elif mutant == "nfull without << 6":
        assert bad == list(range(8, 401)) and ap.permuted_views(8, mutant) is None      # (blocks leave the array)
    elif mutant == "pair from the wrong quotient":
        assert bad == list(range(4, 401))              # 2 S >= 8: the first whole group of (product, view) pairs
    else:
        assert set(range(16, 401)) <= set(bad) and min(bad) == 8
    # the case lists hold a size at which each is wrong
    plans = [(c, ap.bwd_plan(c.S, c.C, c.H * c.W, c.dscore, c.dvdk)) for c in ap.attention_cases()]
    sizes = {c.S for c, d in plans if (d[2] if which == "dvdk" else d[1] or ap.fwd_key(c.S, c.C, c.H * c.W)[1] == "q32")}
    if which == "bgemm":
        assert any(ap.map_faults("bgemm", c.batch, ap.b_plan(c)[2] * ap.b_plan(c)[3], mutant) for c in ap.bgemm_cases() if ap.b_plan(c)[1])
    else:
        assert sizes & set(bad), (mutant, sorted(sizes))


def test_every_reachable_class_is_in_the_case_lists_or_named_over_the_cap():
    """Every class the SMALL / TINY networks reach at S = 1 .. 368, and every bgemm class (key + product) that a product of
    the attention domain or of the linear sweep reaches, has a case that runs THAT product -- through ops.attention
    (attention_cases) or as a direct case with ops' own arguments (bgemm_cases) -- or is named over the cap."""
    attn, lin = ap.model_attention_shapes()
    assert attn == [(64, 64), (192, 256), (320, 64)] and lin == [(32, 128), (64, 256), (128, 32), (256, 64)], (attn, lin)
    assert set(lin) <= set(ap.LIN_SWEEP)
    reached, over = ap.model_classes(), ap.over_cap_classes()
    domain = ap.domain_bgemm_classes()
    covered = ap.attention_covered()
    direct = {ap.b_named_key(c) for c in ap.bgemm_cases()}
    in_cases = lambda k: k in covered or k in direct
    print()
    fmt = lambda k: " | ".join(", ".join(v) if isinstance(v, tuple) else str(v) for v in k)
    for k in sorted(set(reached) | set(domain) | covered | direct | set(over), key=str):
        state = "OVER THE CAP" if k in over else "in the case lists" if in_cases(k) else "NOT COVERED"
        print(f"CLASS | {fmt(k)} | models: {reached.get(k, '-')} | {state}")
    missing = [k for k in list(reached) + list(domain) if not in_cases(k) and k not in over]
    assert not missing, missing
    assert len(domain) >= 100 and {k[-1] for k in domain} == set(ap.PRODUCT_NAMES)
    # the generic maps at whole groups of eight and a remainder, with more than one tile per view (12x12: 9, 32x32: 256)
    assert {(c.S, c.H, c.W) for c in ap.attention_cases()} >= {(S, H, W) for S in (8, 11) for H, W in ((9, 9), (12, 12), (32, 32), (6, 10))}
    # over the cap (S L^2 C > 6e8 at the cheapest shape of the class): named, never dropped silently
    for k, shape in sorted(over.items(), key=str):
        print(f"OVER THE CAP | {fmt(k)} | cheapest shape (S, C, L, dscore, dvdk) {shape}")
    assert {k[:4] for k in over if k[0] == "fwd"} == {("fwd", "128-query", 256, c) for c in ("odd >= 3", "even >= 4", "10")}
    assert all(k[1] == "128-query" for k in over), sorted(over, key=str)


def test_the_case_lists_are_deterministic_capped_and_hold_one_case_per_class():
    cs = ap.attention_cases()
    ap._enumerate.cache_clear()
    assert ap.attention_cases() == cs and len({ap.a_id(c) for c in cs}) == len(cs)
    own = set()
    for c in cs:
        L = c.H * c.W
        assert ap.a_cost(c.S, c.C, L) <= ap.ATTN_CAP, ap.a_id(c)
        keys = set(ap.a_keys(c.S, c.C, L, c.dscore, c.dvdk))
        assert c.why.startswith("edge") or keys - own, (ap.a_id(c), "adds no class")
        own |= keys
    ids = {ap.a_id(c) for c in cs}
    # the edges of the forward's choice, both sides; the generic maps of the issue; every forward kernel at both fused maps
    assert {f"S{S}-C{C}-16x16" for S, C in ap.EDGES} <= ids
    assert {(c.H, c.W) for c in cs} == {(8, 8), (16, 16), (9, 9), (6, 10), (32, 32), (12, 12), (64, 64)}
    assert {k[1:3] for k in own if k[0] == "fwd" and k[1] != "generic"} == {("q16", 64), ("q16", 256), ("q32", 256), ("128-query", 256), ("split", 64)}
    assert {k[2] for k in own if k[0] == "bwd"} == {"dscore+dvdk", "dscore+2 bgemm", "round-4 route", "L = 64", "generic"}
    assert {k[1] for k in own if k[0] == "bwd" and k[2] == "round-4 route"} == {"q16", "q32", "128-query"}
    assert {k[4] for k in own if k[0] == "bwd" and k[4]} == {"2S = 2 < 8", "2S = 4 < 8", "2S = 6 < 8", "2S % 8 = 0", "2S % 8 = 2", "2S % 8 = 4", "2S % 8 = 6"}
    bs = ap.bgemm_cases()
    assert len({ap.b_id(c) for c in bs}) == len(bs) and all(c.batch * c.M * c.N * c.K <= ap.BGEMM_CAP for c in bs)
    keys, named = [ap.b_key(c) for c in bs], [ap.b_named_key(c) for c in bs]
    # one case per (class, product); the alignment term alone has two (A misaligned, B misaligned: one bit of the plan, two
    # ways to miss it)
    assert len(set(named)) == len(named) - 1 and named.count(ap.b_named_key(bs[[c.name for c in bs].index("refused align A")])) == 2
    for axis, want in ((1, set(ap.VARIANT_NAMES)), (8, {"1", "< 8", "8g", "8g + r"}), (4, {"K % 32 = 0", "K % 4 = 0", "K % 4 != 0"})):
        assert {k[axis] for k in keys} == want
    for v in ap.VARIANT_NAMES:                             # per variant: every tail, bias, alpha, beta and batch class
        mine = [k for k in keys if k[1] == v]
        assert {k[2] for k in mine} == {"M tail", "M full"} and {k[3] for k in mine} == {"N tail", "N full"}
        assert {k[5] for k in mine} == {"bias", "no bias"} and {k[6] for k in mine} == {"beta", "beta 0"}
        assert {k[7] for k in mine} == {"alpha", "alpha 1"} and {k[8] for k in mine} >= {"1", "< 8", "8g", "8g + r"}
    assert {k[9] for k in keys if len(k[9]) == 1} == {(n,) for n in ap.REFUSAL_BITS}, "each refusal term alone"
    sm = ap.softmax_cases()
    assert len({ap.softmax_key(*c) for c in sm}) == len(sm) == 32
    assert {c[1] for c in sm} >= {64, 65, 256, 257, 1024, 1025, 4096}


def test_the_softmax_floor_is_four_times_the_largest_reference_error():
    e, floor = ap.softmax_floor()
    print(f"\nSOFTMAX | largest stock fp32 error over the case list {e:.3e} | floor {floor:.0e}")
    assert cr.TOL["softmax"] == pytest.approx(floor, rel=1e-12) and e <= cr.CAP
