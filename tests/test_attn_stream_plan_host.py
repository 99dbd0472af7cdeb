"""The streaming-attention launch plan on the CPU (tests/attn_stream_plan_ref.py against libvf_hip.so and against itself):

  * the restated plan equals vf_attn_stream_plan -- the function vf_attn_stream_fwd / vf_attn_stream_bwd execute -- over
    S = 0 .. 400, C = -1 .. 513, L = 0 .. 520 and 4095, 4096, 4097, 5184, 16384, and the four alignment states of (qkv, dO).
    No field depends on more than (S, L), C alone or (L, alignment), so two slabs hold every combination a field can
    tell apart: every C x every L x every alignment at S in {1, 400}, and every S x every L at C in {0, 1, 513} aligned
    and misaligned (3.4 million plans; the full product would be 434 million calls);
  * ops.attention_route on both sides of STREAM_MIN_L, and _AttentionStreamFn's rowstat / delta sizes against the plan's;
  * the index algebra of the kernels, restated in numpy: crow, put_tile against chan_tiles_mfma, chan_mfma for every
    C <= 512, the waves' channel tiles, ld4 for every L <= 520, block_ids for every ceil(L / 32) <= 600 and S <= 400 (three
    wrong remaps fail);
  * the numpy model of the algorithm as written equals the closed form in float64 on every case, and each of its eight
    wrong variants fails cond_ref.judge on every case it applies to;
  * the case list: deterministic, capped, one case per key, every key of the domain covered, every class the models reach
    at L > 4096 in it."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import attn_stream_plan_ref as sp
import cond_ref as cr

N_CASES, N_KEYS = 100, 115
L_SWEEP = list(range(0, 521)) + [4095, 4096, 4097, 5184, 16384]
ALIGN4 = ((0, 0), (4, 0), (0, 8), (12, 4))


@pytest.fixture(scope="module")
def lib():
    from view_fusion_amd import _lib
    return _lib.load()


def _query(lib, aq, ad, S, C, L):
    """vf_attn_stream_plan at every point (arrays broadcast together) -> ((n, 10) int32, the flat arguments)."""
    args = [np.ascontiguousarray(a).ravel() for a in np.broadcast_arrays(aq, ad, S, C, L)]
    n = args[0].size
    out = np.full((n, 10), -1, dtype=np.int32)
    base = out.ctypes.data
    rcs = list(map(lib.vf_attn_stream_plan, (4096 + args[0]).tolist(), (8192 + args[1]).tolist(), *(a.tolist() for a in args[2:]),
                   range(base, base + 40 * n, 40)))
    assert not any(rcs)
    return out, args


def _compare(lib, aq, ad, S, C, L):
    got, args = _query(lib, aq, ad, S, C, L)
    want = sp.plan_arrays(*args)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (dict(zip(("aq", "ad", "S", "C", "L"), (int(a[bad[0]]) for a in args))), got[bad[0]].tolist(), want[bad[0]].tolist())
    return got.shape[0]


# ------------------------------------------------------------------------------------------------ the plan
def test_the_plan_equals_the_library_over_the_whole_domain(lib):
    al = np.array(ALIGN4, dtype=np.int64)
    Ls, Cs, Ss = np.array(L_SWEEP, dtype=np.int64), np.arange(-1, 514, dtype=np.int64), np.arange(0, 401, dtype=np.int64)
    n = _compare(lib, al[:, 0][:, None, None, None], al[:, 1][:, None, None, None], np.array([1, 400])[None, :, None, None],
                 Cs[None, None, :, None], Ls[None, None, None, :])
    n += _compare(lib, al[::3, 0][:, None, None, None], al[::3, 1][:, None, None, None], Ss[None, :, None, None],
                  np.array([0, 1, 513])[None, None, :, None], Ls[None, None, None, :])
    print(f"\n{n} plans")
    # the scalar restatement is the array one, and says what the issue says
    for a, S, C, L in ((ALIGN4[i % 4], S, C, L) for i, (S, C, L) in enumerate([(1, 1, 1), (3, 192, 4160), (2, 513, 64), (0, 64, 64), (2, 64, 0),
                                                                                (400, 512, 16384), (7, 129, 260), (1, 256, 4225)])):
        assert sp.plan(*a, S, C, L) == sp.plan_arrays(*a, S, C, L).tolist()
    assert sp.plan(0, 0, 3, 192, 4160) == [1, 2, 1, 1, 130, 3, 17, 33, 2 * 3 * 4160, 3 * 4160]
    assert sp.plan(4, 0, 3, 192, 4160)[2:4] == [0, 0] and sp.plan(0, 4, 3, 192, 4160)[2:4] == [1, 0] and sp.plan(0, 0, 1, 256, 4225)[2:4] == [0, 0]
    assert [sp.tiles_per_wave(C) for C in (1, 128, 129, 256, 257, 384, 385, 512)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert sp.plan(0, 0, 0, 64, 64)[0] == sp.plan(0, 0, 2, 64, 0)[0] == sp.plan(0, 0, -1, 0, 64)[0] == sp.EMPTY      # (empty wins over refused)
    assert sp.plan(0, 0, 1, 0, 64)[0] == sp.plan(0, 0, 1, 513, 64)[0] == sp.REFUSED
    # the float counts saturate instead of wrapping
    buf = (ctypes.c_int * 10)()
    assert lib.vf_attn_stream_plan(None, None, 70000, 64, 20000, ctypes.cast(buf, ctypes.c_void_p)) == 0
    assert list(buf) == sp.plan(0, 0, 70000, 64, 20000) and buf[8] == sp.INT_MAX and buf[9] == 1400000000
    assert lib.vf_attn_stream_plan(None, None, 1, 64, 64, None) == 1


def test_the_route_and_the_buffer_sizes_of_ops_agree_with_the_plan(monkeypatch):
    from view_fusion_amd import ops
    mod = importlib.import_module("view_fusion_amd.ops.attention")
    assert mod.STREAM_MIN_L == 4097
    for C in (1, 32, 63, 64, 192, 256, 320, 512):
        for L in (1, 64, 256, 4095, 4096):
            assert ops.attention_route(C, L) != "stream", (C, L)
        for L in (4097, 4098, 4160, 4225, 5184, 16384):
            assert ops.attention_route(C, L) == "stream", (C, L)

    class Spy:                                    # torch, remembering what the autograd function allocates
        def __init__(self):
            self.made = []

        def __getattr__(self, name):
            return getattr(torch, name)

        def empty(self, *a, **k):
            self.made.append(torch.empty(*a, **k))
            return self.made[-1]

        def empty_like(self, *a, **k):
            self.made.append(torch.empty_like(*a, **k))
            return self.made[-1]

    class Ctx:
        def save_for_backward(self, *t):
            self.saved_tensors = t

    calls = []
    monkeypatch.setattr(mod, "_check", lambda *t: None)
    monkeypatch.setattr(mod, "_stream", lambda: None)
    monkeypatch.setattr(mod, "_launch", lambda kind, flops, name, *args, **kw: calls.append((name, args)))
    for S, C, H, W in ((1, 192, 64, 65), (3, 64, 7, 29), (2, 17, 1, 1)):
        L = H * W
        spy = Spy()
        monkeypatch.setattr(mod, "torch", spy)
        del calls[:]
        qkv = torch.zeros(S, 3 * C, H, W)
        ctx = Ctx()
        out = mod._AttentionStreamFn.forward(ctx, qkv, True)
        _, _, rowstat = ctx.saved_tensors
        dqkv, _ = mod._AttentionStreamFn.backward(ctx, torch.zeros(S, C, H, W))
        p = dict(zip(sp.FIELDS, sp.plan(qkv.data_ptr(), 0, S, C, L)))
        assert [n for n, _ in calls] == ["vf_attn_stream_fwd", "vf_attn_stream_bwd"]
        (fa, ba) = (a for _, a in calls)
        assert fa[3:6] == (S, C, L) and ba[6:9] == (S, C, L)
        assert rowstat.numel() == p["rowstat_floats"] and fa[2].value == rowstat.data_ptr() == ba[3].value
        delta = [t for t in spy.made if t.data_ptr() == ba[4].value]
        assert len(delta) == 1 and delta[0].numel() == p["delta_floats"]
        assert out.numel() == S * C * L and dqkv.shape == qkv.shape and ba[5].value == dqkv.data_ptr()
        ctx2 = Ctx()
        mod._AttentionStreamFn.forward(ctx2, qkv, False)
        assert ctx2.saved_tensors[2] is None and calls[-1][1][2] is None


# ------------------------------------------------------------------------------------------------ the index algebra
def test_crow_deals_the_rows_once_and_put_tile_agrees_with_the_read():
    assert sorted(sp.crow(r, lh) for r in range(16) for lh in (0, 1)) == list(range(32))
    for lh in (0, 1):
        for g in range(4):
            for e in range(4):
                assert sp.put_tile_column(g, e, lh) == sp.tiles_read_column(g, e, lh) == sp.crow(4 * g + e, lh)
    # a lane's four registers 4 g .. 4 g + 3 are one aligned float4 of the padded LDS row
    assert all(sp.put_tile_column(g, 0, lh) % 4 == 0 and sp.put_tile_column(g, 3, lh) < sp.SQ <= sp.SPAD for g in range(4) for lh in (0, 1))


def test_chan_mfma_deals_every_channel_once_and_reads_none_past_C():
    for C in range(1, 513):
        summed, addressed = sp.chan_mfma_channels(C)
        assert sorted(summed) == list(range(C)), C
        assert max(addressed) < C and min(addressed) >= 0, C
        assert len(addressed) == 2 * ((C + 1) // 2), C          # one MFMA per channel pair
        dropped, _ = sp.chan_mfma_channels(C, "the last odd channel dropped")
        assert (sorted(dropped) == list(range(C))) == (C % 2 == 0), C


def test_the_waves_tiles_cover_every_channel_tile_once():
    for C in range(1, 513):
        tiles = sp.wave_tiles(C)
        nt, n = sp.tiles_per_wave(C), (C + 31) // 32
        assert sorted(t for w in tiles for t in w) == list(range(n)), C
        assert all(len(w) <= nt for w in tiles) and max(len(w) for w in tiles) == nt and 1 <= nt <= 4, C
        assert all(t == w + 4 * i for w, ts in enumerate(tiles) for i, t in enumerate(ts)), C
        # the stores: row crow(r, lh) of tile ct is channel 32 ct + crow(r, lh); kept iff < C
        stored = sorted(32 * t + sp.crow(r, lh) for w in tiles for t in w for r in range(16) for lh in (0, 1) if 32 * t + sp.crow(r, lh) < C)
        assert stored == list(range(C)), C


def test_ld4_stays_inside_its_row():
    for L in range(1, 521):
        kks = sp.ld4_kk(L)
        assert all(kk % 4 == 0 for kk in kks) and sorted(set(kks)) == list(range(0, 128 * ((L + 127) // 128), 4))
        for vec in ((0, 1) if L % 4 == 0 else (0,)):
            seen = set()
            for kk in kks:
                offs, wide = sp.ld4_addresses(kk, L, vec)
                assert 0 <= min(offs) and max(offs) <= L - 1, (L, kk, vec)
                assert not wide or (offs[0] % 4 == 0 and offs == list(range(kk, kk + 4))), (L, kk, vec)
                seen |= {o for t, o in enumerate(offs) if kk + t < L}
            assert seen == set(range(L)), (L, vec)                 # ... and every entry of the row is read
    # vec with L % 4 != 0 is a state the plan never produces: it would leave the row
    assert max(sp.ld4_addresses(4, 6, 1)[0]) > 5 and sp.plan(0, 0, 1, 8, 6)[2:4] == [0, 0]


def test_block_ids_is_a_bijection_that_keeps_an_xcd_on_consecutive_logical_ids():
    """Every ceil(L / 32) <= 600 and S <= 400: xcd_remap depends on the grid only through nb = gx gy, and maps XCD x's blocks
    onto one interval -- the eight intervals tile [0, nb) for every nb <= 240 000 (checked for all of them at once), so
    id -> (id % gx, id / gx) is a bijection onto (block, view).  The whole map is then run block by block for every grid
    of up to 4096 workgroups and for the edges of the range."""
    assert sp.remap_intervals_tile(600 * 400)
    n = 0
    grids = [(gx, gy) for gx in range(1, 601) for gy in range(1, 401) if gx * gy <= 4096]
    grids += [(gx, gy) for gx in (1, 2, 7, 8, 9, 130, 133, 512, 599, 600) for gy in (1, 2, 3, 7, 8, 9, 16, 17, 399, 400) if gx * gy > 4096]
    for gx, gy in grids:
        assert sp.block_ids_faults(gx, gy) == [], (gx, gy)
        n += 1
    print(f"\n{n} grids run block by block")
    # a view's blocks: consecutive logical ids, on at most ceil(gx / (nb / 8)) + 1 XCDs
    for gx, gy in ((130, 3), (17, 9), (4, 8), (512, 16), (5, 5)):
        blk, b = sp.block_ids(gx, gy)
        q = gx * gy // 8
        for v in range(gy):
            xcds = np.unique(np.nonzero(b == v)[0] % 8)
            assert sorted(blk[b == v]) == list(range(gx)) and xcds.size <= -(-gx // q) + 1, (gx, gy, v)


@pytest.mark.parametrize("mutant", sp.REMAP_MUTANTS)
def test_a_wrong_remap_fails_the_check(mutant):
    grids = [(gx, gy) for gx in range(1, 41) for gy in range(1, 21)]
    bad = [g for g in grids if sp.block_ids_faults(*g, mutant)]
    print(f"\nREMAP MUTANT | {mutant} | wrong at {len(bad)} of {len(grids)} grids, first {bad[:5]}")
    assert bad
    if mutant == "start without the remainder":
        assert all(g[0] * g[1] % 8 for g in bad)          # (right by accident where no XCD holds an extra block)
    elif mutant == "xcd and slot swapped":
        assert all(sp.block_ids_faults(*g, mutant)[0].startswith("XCD") for g in bad) and set(bad) >= {g for g in grids if g[0] * g[1] >= 16}
    else:
        assert all(g[0] != g[1] for g in bad)
    # the case list holds a grid at which each is wrong
    assert any(sp.block_ids_faults((c.L + 31) // 32, c.S, mutant) for c in sp.cases()), mutant


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("c", sp.cases(), ids=sp.c_id)
def test_the_model_equals_the_closed_form_and_every_wrong_model_fails(c):
    qkv, dO, r64, r32 = sp.refs(c)
    got = sp.model(qkv, dO)
    got = [got[0], got[1], got[2][:, 0], got[2][:, 1]]
    for name, a, b in zip(("out", "dqkv", "c2 max", "1 / sum"), got, r64):
        assert cr.err(a, b) <= 1e-12, (name, cr.err(a, b))
    tols = (cr.TOL["attn_fwd"], cr.TOL["attn_bwd"], cr.TOL["attn_fwd"], cr.TOL["attn_fwd"])
    es = [cr.err(a, b) for a, b in zip(r32, r64)]
    assert max(es) <= cr.CAP, es
    applied = 0
    for mutant in sp.MUTANTS:
        if not sp.mutant_applies(mutant, c.S, c.C, c.L):
            continue
        applied += 1
        m = sp.model(qkv, dO, mutant)
        m = [m[0], m[1], m[2][:, 0], m[2][:, 1]]
        which = (0,) if mutant in sp.FWD_MUTANTS else (1, 2, 3) if mutant == sp.BWD_MUTANTS[1] else (1,)
        for i in which:
            d, e, b, ok = cr.judge(m[i], r64[i], r32[i], tols[i])
            assert not ok or (mutant == sp.BWD_MUTANTS[1] and i == 2), (mutant, i, d, b)
        # (the last block's maximum may BE the running one -- attn_input puts a largest key last --, its sum never is)
    assert applied >= 1


def test_every_wrong_model_applies_to_a_case():
    for mutant in sp.MUTANTS:
        hit = [sp.c_id(c) for c in sp.cases() if sp.mutant_applies(mutant, c.S, c.C, c.L)]
        print(f"MODEL MUTANT | {mutant} | applies to {len(hit)} cases")
        assert len(hit) >= 3, mutant


# ------------------------------------------------------------------------------------------------ the case list
def test_the_case_list_is_deterministic_capped_and_holds_one_case_per_key():
    cs = sp.cases()
    sp._enumerate.cache_clear()
    assert sp.cases() == cs and len({sp.c_id(c) for c in cs}) == len(cs)
    own = set()
    for c in cs:
        assert sp.cost(c.S, c.C, c.L) <= sp.ATTN_CAP and 1 <= c.C <= 512, sp.c_id(c)
        mine = set(sp.keys(c.S, c.C, c.L, c.aq, c.ad))
        assert mine - own, (sp.c_id(c), "adds no key")
        own |= mine
    assert own == sp.covered() == sp.all_keys() and sp.over_cap_classes() == {}
    print(f"\n{len(cs)} cases, {len(own)} keys, none over the cap; the dearest case {max(sp.cost(c.S, c.C, c.L) for c in cs):.2e} multiply-adds")
    assert (len(cs), len(own)) == (N_CASES, N_KEYS)
    # the classes of the issue, by name
    assert {k[1] for k in own if k[0] == "chan"} == {1, 2, 3, 4}
    for nt in (1, 2, 3, 4):
        assert {k[2] for k in own if k[0] == "vec" and k[1] == nt} == set(sp.VEC_STATES)
        assert {k[2] for k in own if k[0] == "blocks" and k[1] == nt} == {"1", "2", "3", ">= 4"}
        assert {k[3] for k in own if k[0] == "chan" and k[1] == nt} >= {"all equal", "unequal counts"} - ({"unequal counts"} if nt == 1 else set())
        assert {k[4] for k in own if k[0] == "chan" and k[1] == nt} == {"C % 16 = 0", "even tail", "odd C"}
        assert {k[2] for k in own if k[0] == "chan" and k[1] == nt} == {"last tile full", "last tile partial"}
    assert {k[3] for k in own if k[0] == "chan"} == {"all equal", "unequal counts", "some without a tile"}
    assert {k[5] for k in own if k[0] == "chan"} == {"C = 1", "C < 16", "C >= 16"}
    assert {k[1] for k in own if k[0] == "L"} == {None, "L = 1", "L < 32", "L = 32", "L = 128", "L = 129"}
    assert {(k[2], k[3], k[4]) for k in own if k[0] == "L"} >= {(b, live, r) for b in ("1", "2", "3", ">= 4") for live in (1, 2, 3, 4)
                                                                for r in ("ragged", "whole")}
    assert {k[1:] for k in own if k[0] == "grid"} == {(s, w) for s in ("S = 1", "S > 1") for w in ("< 8", "% 8 = 0", "% 8 != 0")}
    Ls = {c.L for c in cs}
    assert Ls >= {1, 32, 33, 64, 65, 96, 97, 128, 129, 257, 385} and any(c.C < 16 and c.L % 4 and c.L >= sp.MIN_L for c in cs)
    assert any(c.C % 32 and sp.tiles_per_wave(c.C) > 1 and c.L >= sp.MIN_L for c in cs)
    assert {(c.aq, c.ad) for c in cs} == {(0, 0), (4, 0), (0, 4)}


def test_every_class_the_models_reach_above_4096_pixels_is_in_the_case_list():
    reached = sp.model_classes()
    have = sp.covered()
    print()
    for k, shape in sorted(reached.items(), key=str):
        print(f"CLASS | {' | '.join(str(v) for v in k)} | first at (S, C, L) {shape} | {'in the case list' if k in have else 'NOT COVERED'}")
    assert not [k for k in reached if k not in have]
    assert {k[1] for k in reached if k[0] == "chan"} == {1, 2, 3}          # C = 192 takes the <2> instantiations
    assert ("vec", 2, "1/1") in reached and ("vec", 2, "0/0 L % 4 = 1") in reached


def test_the_new_conditioning_shapes_are_what_the_issue_says():
    assert (192, 10, 20, 2) in cr.STREAM_SHAPES and (64, 7, 29, 2) in cr.STREAM_SHAPES
    assert sp.plan(0, 0, 2, 192, 200)[1:4] == [2, 1, 1] and sp.plan(0, 0, 2, 64, 203)[1:4] == [1, 0, 0]
