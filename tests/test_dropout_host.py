"""Seeded residual-block Dropout on the host (csrc/rng.h kind 5, "Dropout masks"): the library's host mirror against the
numpy restatement of tests/dropout_ref.py bit for bit, the threshold identity that makes the integer compare the
existing kernel's `u >= p`, the keep rate, the counter layout written out by hand, the declarations and the argument
errors (raised before anything touches the library).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dropout_ref
import rng_ref
from conftest import ROOT, TINY

SEED = 0xC0FFEE1234567
IDS = [7, 2 ** 32 + 5, 1000003]          # not consecutive, one above 2^32
OFF = [0, 1, 4, 6]                       # view_count = [1, 3, 2]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from view_fusion_amd import _lib
    return _lib.load()


def host_keep(lib, seed, ids, off, n, thr, layer, expect=0):
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    off = np.ascontiguousarray(off, dtype=np.int32)
    S = int(off[-1])
    out = np.full((S, n), 7, dtype=np.uint8)
    rc = lib.vf_dropout_mask_host(seed, ctypes.c_void_p(ids.ctypes.data), ctypes.c_void_p(off.ctypes.data), ids.size, S, n,
                                  thr, layer, ctypes.c_void_p(out.ctypes.data))
    assert rc == expect, rc
    return out


# ---- 1. the host mirror equals the restatement -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1036])
@pytest.mark.parametrize("layer", [0, 37])
@pytest.mark.parametrize("p", [0.1, 0.25])
def test_host_mirror_equals_the_restatement(lib, p, layer, n):
    from view_fusion_amd import ops
    thr, scale = ops.dropout_constants(p)
    assert thr == dropout_ref.threshold(p)
    assert np.float32(scale).view(np.uint32) == dropout_ref.scale(p).view(np.uint32)
    got = host_keep(lib, SEED, IDS, OFF, n, thr, layer)
    want = dropout_ref.keep(SEED, IDS, OFF, n, p, layer)
    assert got.shape == want.shape == (6, n) and set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), want)
    if n == 1036:                                    # a real mask, and no two rows alike
        assert 0.5 < want.mean() < 0.99 and len({r.tobytes() for r in want}) == 6


def test_host_mirror_refusals(lib):
    ok = dict(seed=SEED, ids=IDS, off=OFF, n=8, thr=5, layer=0)
    for bad in (dict(n=6), dict(thr=2 ** 24 + 1), dict(layer=65536), dict(layer=-1), dict(off=[0, 1, 4, 4]),
                dict(off=[0, 4096])):
        kw = dict(ok, **bad)
        if bad.get("off") == [0, 4096]:
            kw["ids"] = [1]
        host_keep(lib, expect=1, **kw)               # hipErrorInvalidValue
    assert host_keep(lib, **dict(ok, thr=2 ** 24)).sum() == 0 and host_keep(lib, **dict(ok, thr=0)).all()
    assert host_keep(lib, SEED, [1], [0, 4095], 4, 0, 65535).all()           # the largest view count and layer pass


# ---- 2. the threshold identity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.2, 0.25, 0.3, 0.5, 0.999])
def test_threshold_identity(p):
    from view_fusion_amd import ops
    thr = ops.dropout_constants(p)[0]
    assert thr == dropout_ref.threshold(p) and 0 < thr <= 2 ** 24
    k = np.concatenate([np.arange(thr - 2, thr + 3), np.random.default_rng(1).integers(0, 2 ** 24, 100000)])
    k = k[(k >= 0) & (k < 2 ** 24)].astype(np.int64)
    u = (k.astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    assert np.array_equal(u.astype(np.float64), k * 2.0 ** -24)              # u = k 2^-24 is exact in fp32
    assert np.array_equal(k >= thr, u >= np.float32(p))
    assert (k >= thr).any() and not (k >= thr).all()


def test_p_zero_keeps_everything(lib):
    from view_fusion_amd import ops
    assert ops.dropout_constants(0.0) == (0, 1.0) and dropout_ref.threshold(0.0) == 0
    assert host_keep(lib, SEED, IDS, OFF, 1036, 0, 3).all()
    assert dropout_ref.keep(SEED, IDS, OFF, 1036, 0.0, 3).all()
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            ops.dropout_constants(bad)


# ---- 3. the keep rate ------------------------------------------------------------------------------------------------
def test_keep_rate(lib):
    p, n = 0.1, 2 ** 20
    thr = dropout_ref.threshold(p)
    got = host_keep(lib, 2024, [11], [0, 1], n, thr, 5)
    want = 1.0 - thr / 2.0 ** 24
    sigma = (p * (1 - p) / n) ** 0.5
    print(f"kept {got.mean():.6f} of {n} draws, stated {want:.6f}: {(got.mean() - want) / sigma:+.2f} sigma")
    assert abs(got.mean() - want) <= 5 * sigma
    assert abs(want - (1 - p)) <= 2.0 ** -24 + abs(float(np.float32(p)) - p)  # thr / 2^24 - float32(p) < 2^-24


# ---- 4. the counter layout -------------------------------------------------------------------------------------------
def _by_hand(seed, id_, layer, view, block):
    ctr = (block, id_ & 0xFFFFFFFF, id_ >> 32, (5 << 28) | (layer << 12) | view)
    return rng_ref.philox_int(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def test_counter_layout(lib):
    base = dict(seed=SEED, id_=2 ** 32 + 5, layer=3, view=2, block=9)
    w0 = _by_hand(**base)
    assert tuple(int(x) for x in dropout_ref.counter_words(SEED, base["id_"], 3, 2, 9)) == w0
    seen = {w0}
    for k, v in (("seed", SEED + 1), ("seed", SEED + 2 ** 32), ("id_", 2 ** 32 + 6), ("id_", 5), ("view", 3),
                 ("layer", 4), ("block", 10)):
        w = _by_hand(**dict(base, **{k: v}))
        assert all(a != b for a, b in zip(w, w0)), k                          # every one of the four words changes
        seen.add(w)
    assert len(seen) == 8
    # view and layer share no bit of the step: (layer 1, view 0) would be (layer 0, view 4096), which is refused
    assert (1 << 12) | 0 == (0 << 12) | 4096
    with pytest.raises(ValueError):
        dropout_ref.keep(SEED, [1], [0, 4097], 4, 0.5, 0)
    host_keep(lib, SEED, [1], [0, 4097], 4, 5, 0, expect=1)
    assert _by_hand(SEED, 1, 1, 0, 0) != _by_hand(SEED, 1, 0, 4095, 0)
    # the library's mirror on exactly that counter: row 2 of sample 1 (view 2 - off = ...) at layer 3, block 9
    thr = dropout_ref.threshold(0.5)
    got = host_keep(lib, SEED, IDS, OFF, 40, thr, 3)
    assert got[3, 36:40].tolist() == [int((w >> 8) >= thr) for w in w0]       # row 3 = view 2 of sample 1 (id 2^32 + 5)


# ---- declarations, numbering, argument errors ------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound():
    from view_fusion_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    for name in ("vf_dropout_seeded", "vf_dropout_mask_host"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, f"{name} is not declared in include/vf_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.SIGNATURES["vf_dropout"] == [ctypes.c_void_p] * 3 + [ctypes.c_long, ctypes.c_float, ctypes.c_void_p]
    assert callable(ops.dropout_seeded)
    src = open(os.path.join(ROOT, "view_fusion_amd", "csrc", "rng.h")).read()
    assert "VF_RNG_DROPOUT = 5" in src and "vf_rng_dropout_keep" in src


def test_blocks_are_numbered_in_execution_order_and_state_dict_is_unchanged():
    from view_fusion_amd import UNet
    from view_fusion_amd.unet import _ResAttnBlock
    plain, drop = UNet(**TINY), UNet(**dict(TINY, dropout=0.25))
    assert list(plain.state_dict()) == list(drop.state_dict())
    blocks = [m for m in list(drop.downs) + list(drop.mid) + list(drop.ups) if isinstance(m, _ResAttnBlock)]
    assert [m.res_block._vf_layer for m in blocks] == list(range(len(blocks))) and len(blocks) == 8
    assert not any("_vf_layer" in k for k in drop.state_dict())


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from view_fusion_amd import _lib, ops

    def boom(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "call", boom)
    with pytest.raises(_lib.VFHipError):             # CPU tensors: no fallback
        ops.dropout_seeded(torch.zeros(2, 4), 0.5, 1, torch.zeros(1, dtype=torch.int64), torch.tensor([0, 2]), 0)
