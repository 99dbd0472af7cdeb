"""The one-launch sampler convolutions' plan on the CPU: tests/conv_small_plan_ref.py's restatement equals the host functions
of libvf_hip.so (all sixteen fields of vf_conv_small_plan, vf_conv_small_supported, vf_conv_small_pack_floats) and the policy
of ops (use_small_conv, can_fold_residual) at the natural thresholds and one either side of each; the index algebra of the
kernels, restated as numpy, deals every product exactly once; every class the SMALL / TINY sampler layers reach has a case
in conv_small_plan_ref.cases() -- the list tests/test_gpu_conv_small_plan.py runs -- under the cost cap; and the comparison
rule of those tests rejects seven wrong models on every case they apply to.

vf_conv_small_plan reports conv_small_plan, the function conv_small_launch (behind vf_conv_small, vf_conv_small_res and
vf_conv_small_gn) executes, so pinning it pins the launch.

The sweep (one library call per point; the full product of the axes is out of reach, so every axis is crossed with the
ones the code lets it interact with):
  * sizes: every Cin of the grid x KS {1, 3, 5} x mode {0, 1, 2} x 17 maps (the seven square powers of two, 1, 256, and
    non-square / non-power-of-two ones), at four (S, Cout) -- validity, n, nr and the last round are functions of Cin;
  * grid: S = 0 ... 64 x every Cout of the grid x the square maps x KS {1, 3} x packed -- RS and the grid are functions of
    (S, Cout, H W);
  * operands: every combination of the nine presence flags (512) x twelve (KS, mode, H, Cin, C1, groups, rC1, rC) rows that
    sit on the edges the refusal branches test -- all fifteen refusal codes and the accepted call occur --, and the
    GroupNorm and fold limits over every Cin / rC of the grid.
The grid of channel counts: every multiple of 4 up to 1056 and the +-1 neighbours of the multiples of 16."""
import itertools

import numpy as np
import pytest
import torch

import cond_ref as cr
import conv_small_plan_ref as sp

GRID = np.array(sorted(set(range(4, 1057, 4)) | {m + d for m in range(16, 1057, 16) for d in (-1, 1)} | {1, 2, 3}), dtype=np.int64)
MAPS = [(h, h) for h in (1, 2, 4, 8, 16, 32, 64, 128, 256)] + [(4, 8), (8, 4), (6, 6), (12, 12), (16, 32), (24, 24), (10, 20), (0, 0)]
SQUARE = (4, 8, 16, 32, 64, 128)
ZERO = dict(x2=0, C1=0, ist=0, affine=0, groups=0, ost=0, rx=0, rx2=0, rC1=0, rC=0, rw=0, residual=0, wp=0)


@pytest.fixture(scope="module")
def lib():
    from view_fusion_amd import _lib
    return _lib.load()


def _compare(lib, label, **kw):
    args = dict(zip(sp.ARGS, (np.ascontiguousarray(a).ravel() for a in np.broadcast_arrays(*(np.asarray(kw[k], dtype=np.int64) for k in sp.ARGS)))))
    n = args["S"].size
    out = np.full((n, 16), -1, dtype=np.int32)
    base = out.ctypes.data
    rcs = list(map(lib.vf_conv_small_plan, *(args[k].tolist() for k in sp.ARGS), range(base, base + 64 * n, 64)))
    assert not any(rcs)
    d = sp.plan_arrays(**args)
    want = np.stack([d[k] for k in sp.FIELDS], 1)
    bad = np.nonzero((out != want).any(1))[0]
    assert bad.size == 0, (label, {k: int(v[bad[0]]) for k, v in args.items()}, dict(zip(sp.FIELDS, out[bad[0]].tolist())),
                           dict(zip(sp.FIELDS, want[bad[0]].tolist())))
    return out, args


def test_plan_restatement_equals_the_library_over_the_sizes(lib):
    H = np.array([m[0] for m in MAPS])[None, None, None, :, None]
    W = np.array([m[1] for m in MAPS])[None, None, None, :, None]
    sc = np.array([(1, 5), (2, 32), (7, 100), (64, 1056)])
    out, args = _compare(lib, "sizes", **dict(ZERO, S=sc[None, None, None, None, :, 0], Cout=sc[None, None, None, None, :, 1],
                                              Cin=GRID[:, None, None, None, None], KS=np.array([1, 3, 5])[None, :, None, None, None],
                                              mode=np.array([0, 1, 2])[None, None, :, None, None], H=H, W=W))
    sup = np.array(list(map(lib.vf_conv_small_supported, *(args[k].tolist() for k in ("Cin", "Cout", "H", "W", "KS", "mode")))))
    assert np.array_equal(sup, sp.supported(*(args[k] for k in ("Cin", "Cout", "H", "W", "KS", "mode"))))
    assert np.array_equal(sup == 0, out[:, 0] == 1)
    assert set(out[:, 1].tolist()) == {sp.K_NONE, sp.K_1X1, sp.K_3X3} and set(out[out[:, 1] == 3, 9].tolist()) == {4, 8}
    # the same sizes with every optional operand of a 3x3 / 1x1 call present
    full = dict(ZERO, ost=1, wp=1)
    _compare(lib, "sizes, stats + packed", **dict(full, S=3, Cout=40, Cin=GRID[:, None, None], KS=np.array([1, 3])[None, :, None],
                                                  mode=0, H=np.array(SQUARE)[None, None, :], W=np.array(SQUARE)[None, None, :]))


def test_plan_restatement_equals_the_library_over_the_grids(lib):
    S = np.arange(0, 65)[:, None, None, None, None]
    Hs = np.array(SQUARE)[None, None, :, None, None]
    out, _ = _compare(lib, "grid", **dict(ZERO, S=S, Cout=GRID[None, :, None, None, None], H=Hs, W=Hs, Cin=64, mode=0,
                                          KS=np.array([1, 3])[None, None, None, :, None], wp=np.array([0, 1])[None, None, None, None, :]))
    run = out[out[:, 1] == sp.K_3X3]
    assert {(r[2], r[3], r[4]) for r in run.tolist()} == set(itertools.product((4, 3, 2), (1, 2), (0, 1)))      # all twelve
    _compare(lib, "grid, negative S", **dict(ZERO, S=np.array([-5, -1, 0]), Cout=32, H=16, W=16, Cin=64, KS=3, mode=0))
    for Cout, Cin in ((1, 32), (31, 32), (32, 64), (33, 96), (1056, 1056), (5, 40), (5, 31)):
        assert lib.vf_conv_small_pack_floats(Cout, Cin) == int(sp.pack_floats(Cout, Cin))
    co, ci = np.meshgrid(GRID, np.arange(32, 1057, 32), indexing="ij")
    got = np.array(list(map(lib.vf_conv_small_pack_floats, co.ravel().tolist(), ci.ravel().tolist())))
    assert np.array_equal(got, sp.pack_floats(co.ravel(), ci.ravel()))


def test_plan_restatement_equals_the_library_over_the_operands(lib):
    flags = ("x2", "ist", "affine", "ost", "rx", "rx2", "rw", "residual", "wp")
    combos = np.array(list(itertools.product((0, 1), repeat=len(flags))), dtype=np.int64)
    # (KS, mode, H, Cin, C1, groups, rC1, rC): on the edges the refusal branches test
    rows = np.array([(3, 0, 4, 32, 8, 8, 4, 8), (1, 0, 4, 8, 3, 2, 5, 12), (1, 0, 4, 8, 0, 0, 0, 0), (1, 0, 4, 8, 8, 3, 8, 8),
                     (3, 2, 8, 64, 0, 5, 0, 4), (3, 0, 8, 64, 0, 8, 8, 8), (3, 0, 8, 96, -1, -2, -1, 6), (3, 0, 16, 512, 1, 32, 1, 2), (3, 0, 16, 544, 1, 32, 3, 4),
                     (1, 0, 16, 1024, 1023, 32, 515, 516), (1, 0, 16, 1028, 1028, 4, 516, 516), (5, 0, 8, 32, 4, 8, 4, 8)], dtype=np.int64)
    kw = {k: combos[:, None, i] for i, k in enumerate(flags)}
    out, _ = _compare(lib, "operands", S=2, Cout=20, W=rows[None, :, 2], H=rows[None, :, 2], KS=rows[None, :, 0], mode=rows[None, :, 1],
                      Cin=rows[None, :, 3], C1=rows[None, :, 4], groups=rows[None, :, 5], rC1=rows[None, :, 6], rC=rows[None, :, 7], **kw)
    assert set(out[:, 0].tolist()) == set(range(16)), "every refusal branch and the accepted call are in the sweep"
    # the limits of GroupNorm on load and of the fold, over every channel count
    for KS in (1, 3):
        _compare(lib, "gn limits", **dict(ZERO, S=1, Cout=5, H=4, W=4, KS=KS, mode=0, Cin=GRID[:, None], ist=1, affine=1,
                                          groups=np.array([1, 2, 3, 4, 32])[None, :]))
    _compare(lib, "fold limits", **dict(ZERO, S=1, Cout=5, H=4, W=4, KS=3, mode=0, Cin=32, rx=1, rw=1, rC=GRID[:, None, None],
                                        rx2=np.array([0, 1])[None, :, None], rC1=np.array([0, 1, 4, 515, 1055, 1056])[None, None, :]))
    for code, c, over in sp.REJECTIONS:
        assert sp.plan(c, **over)["code"] == code, (code, sp.case_id(c), over)
    assert {r[0] for r in sp.REJECTIONS} == set(sp.REFUSALS)
    assert lib.vf_conv_small_plan(*([1] * 20), None) == sp.INVALID


def test_policy_restatement_equals_ops_at_and_around_the_natural_thresholds():
    from view_fusion_amd import ops
    nat = dict(wgs1=ops.st.SMALL_CONV_MAX_WGS[0], wgs3=ops.st.SMALL_CONV_MAX_WGS[1], cin3=ops.st.SMALL_CONV_MAX_CIN3, s3=ops.st.SMALL_CONV_MAX_S3)
    assert nat == sp.NATURAL, "the natural thresholds of ops.state"
    saved = ops.st.SMALL_CONV_MAX_WGS, ops.st.SMALL_CONV_MAX_CIN3, ops.st.SMALL_CONV_MAX_S3
    settings = [nat] + [dict(nat, **{k: nat[k] + d}) for k in nat for d in (-1, 1)] + [sp.OPEN]
    # shapes on each threshold and one either side: workgroups = S ceil(Cout / 32) H W / 16
    shapes = [(S, Cin, Cout, H, KS, m) for S in (1, 2, 3, 4, 5, 24) for Cin in (32, 64, 252, 256, 260, 288, 30) for Cout in (6, 32, 33, 64, 65, 1024, 1056)
              for H in (2, 4, 16, 32, 64, 128) for KS in (1, 3) for m in (0, 1, 2)]
    shapes += [(1, 64, 32 * k, 16, KS, 0) for k in (31, 32, 33, 63, 64, 65) for KS in (1, 3)] + [(3, 64, 32 * 21 + d, 64, 1, 0) for d in (-32, 0, 1)]
    took = set()
    try:
        with torch.no_grad():
            for thr in settings:
                ops.st.SMALL_CONV_MAX_WGS, ops.st.SMALL_CONV_MAX_CIN3, ops.st.SMALL_CONV_MAX_S3 = (thr["wgs1"], thr["wgs3"]), thr["cin3"], thr["s3"]
                for s in shapes:
                    want = sp.use_small(*s[:4], s[3], *s[4:], thr=thr)
                    assert bool(ops.use_small_conv(*s[:4], s[3], *s[4:])) == want, (thr, s)
                    took.add(want)
                for S, C, H, rC in itertools.product((1, 2), (64, 256, 260), (16, 64, 128), (4, 6, 64, None)):
                    res = torch.nn.Identity() if rC is None else torch.nn.Conv2d(rC, C, 1)
                    assert bool(ops.can_fold_residual(S, C, H, H, res)) == sp.can_fold(S, C, H, H, rC, thr), (thr, S, C, H, rC)
            with torch.enable_grad():
                assert not ops.can_fold_residual(1, 64, 16, 16, torch.nn.Conv2d(64, 64, 1))
    finally:
        ops.st.SMALL_CONV_MAX_WGS, ops.st.SMALL_CONV_MAX_CIN3, ops.st.SMALL_CONV_MAX_S3 = saved
    assert took == {True, False}


# ------------------------------------------------------------------------------------------------ index algebra
def test_the_two_shift_divisions():
    k = np.arange(144)
    assert np.array_equal((k * 57) >> 9, k // 9)
    t = np.arange(9)
    assert np.array_equal((t * 11) >> 5, t // 3)


def test_conv3_slots_cover_every_product_exactly_once():
    """(wave, round, group q, quarter kk, e) -> (channel, tap): the kept slots are every product of the OIHW row once, the
    weight load and the B table agree on (channel, tap), the dropped slots are exactly the products past the round, and every
    load -- kept or not -- stays inside the row."""
    for Cin in range(32, 1025, 32):
        m = sp.conv3_map(Cin)
        v = m["valid"]
        assert np.array_equal(v, m["k"] < m["np"]), Cin
        flat = m["wch"][v] * 9 + m["wtap"][v]
        assert np.array_equal(np.sort(flat), np.arange(Cin * 9)), Cin
        assert np.array_equal(m["off"][v], flat), Cin
        assert np.array_equal(m["bch"][v], m["wch"][v]) and np.array_equal(m["btap"][v], m["wtap"][v]), Cin
        assert np.array_equal(m["dy"][v] * 3 + m["dx"][v], m["wtap"][v]) and m["dx"].max() == 2 and m["dy"].max() == 2
        assert m["off"].min() >= 0 and m["off"].max() < Cin * 9, Cin      # (the re-read of group 0 past the round's products)
        # a dropped slot addresses a channel of the round that was staged (zero or not): a valid LDS address
        assert ((m["bch"] - (m["wave"] * (Cin >> 3) + 8 * m["round"])) < 8).all()


def test_conv1_and_fold_slots_cover_every_channel_exactly_once():
    for K in range(4, 2049, 4):
        m = sp.conv1_map(K)
        ok = m["ok"]
        assert np.array_equal(np.sort(m["k"][ok]), np.arange(K)), K
        assert np.array_equal(m["load"][ok], m["k"][ok]), K
        assert m["load"].min() >= 0 and m["load"].max() < K, K                # (the K - 4 clamp)
        assert m["n"] % 16 == 0 and 8 * m["n"] >= K > 8 * (m["n"] - 16), K
        assert not (ok & ~m["issued"]).any()
    assert sp.conv1_map(4)["load"].max() == 3 and sp.conv1_map(516)["trips"] == 2 and sp.conv1_map(512)["trips"] == 1


def test_pack_layout_against_oihw():
    rng = np.random.default_rng(3)
    for Cout, Cin in ((5, 32), (16, 64), (33, 96), (40, 160), (64, 128)):
        w = rng.standard_normal((Cout, Cin, 3, 3)).astype(np.float32) + 3.0        # (no zeros of its own)
        packed, src = sp.pack_numpy(w)
        assert packed.size == int(sp.pack_floats(Cout, Cin))
        assert np.array_equal(np.sort(src[src >= 0]), np.arange(w.size)), "every OIHW float exactly once"
        assert np.array_equal(packed == 0, src < 0), "zeros past the round and past Cout, nowhere else"
        # what conv3_small_kernel<., RS, true> reads where the unpacked kernel reads W[co][c0 9 + r 72 + 16 q + 4 kk + e]
        m = sp.conv3_map(Cin)
        p4, flat = packed.reshape(-1, 4), w.reshape(Cout, -1)
        for RS in (1, 2):
            for cot in range((Cout + 16 * RS - 1) // (16 * RS)):
                for rs in range(RS):
                    for j in (0, 7, 15):
                        co = cot * 16 * RS + 16 * rs + j
                        idx = sp.packed_read_index(Cout, Cin, RS, cot, rs, m["wave"], m["round"], m["q"], 16 * m["kk"] + j)
                        assert idx.max() < p4.shape[0]
                        got = p4[idx, m["e"]]
                        want = np.where(m["valid"] & (co < Cout), flat[min(co, Cout - 1)][m["off"]], 0)
                        assert np.array_equal(got, want), (Cout, Cin, RS, cot, rs, j)


def test_tile_and_patch_coordinates():
    rng = np.random.default_rng(4)
    for W in (4, 8, 16, 32, 64):
        for up in ((False, True) if W >= 8 else (False,)):
            g = sp.tile_geometry(W, up)
            assert g["logtc"] == (4 if W >= 16 else 3 if W == 8 else 2) and g["PS"] in (54, 40, 36) and g["PS"] <= 64
            assert np.array_equal(g["pix"].ravel(), np.arange(W * W)), "a tile's 16 pixels are consecutive; every pixel once"
            Ws = W // 2 if up else W
            x = rng.standard_normal((Ws, Ws))
            full = np.kron(x, np.ones((2, 2))) if up else x
            padded = np.pad(full, 1)                              # (the padding is padding of the UPSAMPLED map)
            stored = np.concatenate([x.ravel(), [0.0]])
            for pt in range(W * W // 16):
                patch = stored[g["src"][pt]]                      # what the wave stages (index -1: the zero)
                for j in range(16):
                    oy, ox = divmod(int(g["pix"][pt][j]), W)
                    assert np.array_equal(patch[g["tap"][j]], padded[oy:oy + 3, ox:ox + 3]), (W, up, pt, j)
                assert g["tap"].max() < g["PS"]


# ------------------------------------------------------------------------------------------------ the case list
def test_every_case_is_under_the_cost_cap_and_runs():
    cs = sp.cases()
    assert len({sp.case_id(c) for c in cs}) == len(cs)
    for c in cs:
        assert sp.cost(c) <= sp.MAX_COST, (sp.case_id(c), sp.cost(c))
        d = sp.plan(c)
        assert d["code"] == 0 and d["kernel"] != sp.K_NONE, sp.case_id(c)
    print(f"\n{len(cs)} cases, the most expensive {max(sp.cost(c) for c in cs):.2e} multiply-adds, {sum(sp.cost(c) for c in cs):.2e} in all")


def test_every_required_class_has_a_case():
    assert sp.over_cap_classes() == []
    have = sp.case_classes()
    insts = {k for k in have if k[0] == "inst"}
    assert len([k for k in insts if k[1] == "3x3"]) == 12 and {k[1] for k in insts} == {"1x1", "cat", "3x3"}
    assert {sp.entry(c) for c in sp.cases()} == {"vf_conv_small", "vf_conv_small_res", "vf_conv_small_gn"}
    assert any(c.packed for c in sp.cases()), "the pack kernel runs"


def test_each_case_is_the_cheapest_of_its_classes():
    """No candidate of the generated domain with the same key is cheaper than the key's case."""
    best = {}
    for c in sp.cases():
        for k in sp.class_keys(c):
            best[k] = min(best.get(k, float("inf")), sp.cost(c))
    for c in sp._candidates():
        for k in sp.class_keys(c):
            assert sp.cost(c) >= best[k], (k, sp.case_id(c))


@pytest.mark.parametrize("thr", [sp.NATURAL, sp.OPEN], ids=["natural", "open"])
def test_every_class_the_sampler_layers_reach_has_a_case(thr):
    layers = sp.model_layers()
    assert len(layers) > 20
    reached = sp.reached_classes(thr)
    missing = {k: v for k, v in reached.items() if k not in sp.case_classes()}
    assert not missing, missing
    kinds = {k[1] for k in reached if k[0] == "inst"}
    assert kinds == {"1x1", "cat", "3x3"}, kinds
    print(f"\n{len(reached)} classes reached of {len(sp.case_classes())} covered")
    for k in sorted(reached, key=repr):
        print("REACHED |", thr is sp.NATURAL and "natural" or "open", "|", k, "| first by", reached[k])


# ------------------------------------------------------------------------------------------------ the rule and wrong models
@pytest.mark.parametrize("c", sp.cases(), ids=sp.case_id)
def test_the_rule_rejects_every_wrong_model(c):
    """On the inputs the GPU test uses: the stock fp32 error is under the cap (cond_ref.bound asserts), and each wrong model
    that applies to the case fails err <= max(4 e, tol)."""
    t = sp.inputs(c)
    r64, r32 = sp.refs(c, t)
    err, e, bound, ok = cr.judge(r32, r64, r32, sp.tol(c))
    assert ok and e <= sp.tol(c), (e, bound)
    for m in sp.MUTANTS:
        if sp.mutant_applies(c, m):
            err, _, bound, ok = cr.judge(sp.reference(c, t, torch.float32, m), r64, r32, sp.tol(c))
            print(f"SMALLPLAN-MUTANT | {sp.case_id(c)} | {m} | err {err:.3e} | bound {bound:.3e}")
            assert not ok, (m, err, bound)


def test_every_wrong_model_is_exercised():
    for m in sp.MUTANTS:
        assert any(sp.mutant_applies(c, m) for c in sp.cases()), m
