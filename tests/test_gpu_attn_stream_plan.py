"""Every launch plan class of the streaming self-attention kernels (csrc/attention_stream.hip) on a real MI355X against
float64 (case list, class keys, references and the numpy model: tests/attn_stream_plan_ref.py; the plan itself, the index
algebra and the wrong models are held on the CPU in tests/test_attn_stream_plan_host.py).

  (a) every case through the C ABI: the plan queried on the real addresses, vf_attn_stream_fwd with and without rowstat
      (out bit-identical), vf_attn_stream_bwd; out and d(qkv) against float64, rowstat's two rows (c2 max, 1 / sum) against
      float64 on their own; the backward a second time on out and rowstat made in float64 and rounded once (a wrong
      forward is then told from a wrong backward); all four buffers NaN-filled between two sentinel bands; run 2 = run 1
      bit for bit; a misaligned case = the aligned run of the same values bit for bit; refusals and empty calls write
      nothing;
  (b) through ops: ops.attention_streaming at one shape per NT, ops.attention at the two smallest natural-route shapes of
      the <2> instantiations (L = 4160 vectorised, L = 4225 scalar loads; over ATTN_CAP because the route starts at 4097).

One rule (cond_ref.judge): err = max|a - r64| / max|r64|, e = the same for stock fp32 torch on the CPU, pass if
err <= max(4 e, tol), tol = cond_ref.TOL (attn_fwd 2e-5 for out and rowstat, attn_bwd 5e-5 for d(qkv)); e <= cond_ref.CAP
asserted; a non-finite value fails.  Measured values: profiles/attn_stream_plan.md."""
import ctypes
import math

import pytest
import torch

import attn_stream_plan_ref as sp
import cond_ref as cr
from test_gpu_conditioning import _Log

pytestmark = pytest.mark.gpu

BAND, SENTINEL = 1024, 12345.0
INVALID = 1                                    # hipErrorInvalidValue
TOLS = (cr.TOL["attn_fwd"], cr.TOL["attn_bwd"], cr.TOL["attn_fwd"], cr.TOL["attn_fwd"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from view_fusion_amd import _lib
    return _lib.load()


def _judge_all(label, names, got, r64, r32, tols):
    """Print every figure, then assert the rule for every output."""
    rows = [(n, *cr.judge(a, b, c, t)) for n, a, b, c, t in zip(names, got, r64, r32, tols)]
    print()
    for n, d, e, b, ok in rows:
        print(f"ATTNSTREAM | {label} | {n} | e {e:.3e} | err {d:.3e} | bound {b:.3e} | {'ok' if ok else 'FAIL'}")
    assert all(r[4] for r in rows), [(r[0], r[1], r[3]) for r in rows if not r[4]]


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _banded(dev, *shape):
    """-> (NaN-filled tensor of `shape`, the whole buffer: a sentinel band in front of it and one behind)."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * BAND,), SENTINEL, device=dev)
    buf[BAND:BAND + n] = float("nan")
    return buf[BAND:BAND + n].view(*shape), buf


def _intact(*bufs):
    torch.cuda.synchronize()
    return all(bool((b[:BAND] == SENTINEL).all()) and bool((b[-BAND:] == SENTINEL).all()) for b in bufs)


def _placed(t, dev, off_bytes):
    """t on the device, off_bytes past a 16-byte boundary (torch's allocations are at least 256-byte aligned)."""
    buf = torch.zeros(t.numel() + 4, device=dev)
    assert buf.data_ptr() % 16 == 0 and off_bytes % 4 == 0
    v = buf[off_bytes // 4:off_bytes // 4 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off_bytes
    return v


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(lib, dev, qd, dd, S, C, L, out_in=None, stat_in=None):
    """One forward with rowstat, one without, one backward, each into NaN-filled banded buffers -> (out, rowstat, delta,
    dqkv, out of the call without rowstat); out_in / stat_in: the backward reads these instead of the forward's own."""
    out, b0 = _banded(dev, S, C, L)
    stat, b1 = _banded(dev, S, 2, L)
    out2, b2 = _banded(dev, S, C, L)
    delta, b3 = _banded(dev, S, L)
    dqkv, b4 = _banded(dev, S, 3 * C, L)
    assert lib.vf_attn_stream_fwd(_P(qd), _P(out), _P(stat), S, C, L, _stream()) == 0
    assert lib.vf_attn_stream_fwd(_P(qd), _P(out2), None, S, C, L, _stream()) == 0
    assert lib.vf_attn_stream_bwd(_P(qd), _P(out if out_in is None else out_in), _P(dd), _P(stat if stat_in is None else stat_in),
                                  _P(delta), _P(dqkv), S, C, L, _stream()) == 0
    assert _intact(b0, b1, b2, b3, b4), "a sentinel band was written"
    for name, t in (("out", out), ("rowstat", stat), ("delta", delta), ("dqkv", dqkv), ("out (rowstat null)", out2)):
        assert not bool(torch.isnan(t).any()), f"{name}: an element was left unwritten (or is NaN)"
    return out, stat, delta, dqkv, out2


# ------------------------------------------------------------------------------------------------ (a) the C ABI
@pytest.mark.parametrize("c", sp.cases(), ids=sp.c_id)
def test_stream_plan_class_vs_fp64(dev, lib, c):
    S, C, L = c.S, c.C, c.L
    qkv, dO, r64, r32 = sp.refs(c)
    qd, dd = _placed(qkv, dev, c.aq), _placed(dO, dev, c.ad)
    buf = (ctypes.c_int * 10)()
    assert lib.vf_attn_stream_plan(_P(qd), _P(dd), S, C, L, ctypes.cast(buf, ctypes.c_void_p)) == 0
    plan = dict(zip(sp.FIELDS, buf))
    assert list(buf) == sp.plan(qd.data_ptr(), dd.data_ptr(), S, C, L) == sp.plan(c.aq, c.ad, S, C, L), list(buf)
    assert plan["state"] == sp.RUNS and plan["rowstat_floats"] == 2 * S * L and plan["delta_floats"] == S * L
    if L >= sp.MIN_L:
        assert ("vec", plan["NT"], sp.vec_state(c.aq, c.ad, L)) in sp.keys(S, C, L, c.aq, c.ad)
        assert (plan["vec_fwd"], plan["vec_bwd"]) == {"1/1": (1, 1), "1/0": (1, 0), "0/0": (0, 0)}[sp.vec_state(c.aq, c.ad, L)[:3]]

    out, stat, delta, dqkv, out2 = _run(lib, dev, qd, dd, S, C, L)
    assert torch.equal(_bits(out), _bits(out2)), "out differs between rowstat given and rowstat null"
    again = _run(lib, dev, qd, dd, S, C, L)
    for name, a, b in zip(("out", "rowstat", "delta", "dqkv"), (out, stat, delta, dqkv), again):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: run 2 differs from run 1"
    if c.aq or c.ad:                                    # ld4 changes the width of the loads and no arithmetic
        aligned = _run(lib, dev, _placed(qkv, dev, 0), _placed(dO, dev, 0), S, C, L)
        for name, a, b in zip(("out", "rowstat", "delta", "dqkv"), (out, stat, delta, dqkv), aligned):
            assert torch.equal(_bits(a), _bits(b)), f"{name}: the misaligned run differs from the aligned one"

    label = f"{sp.c_id(c)} NT {plan['NT']} vec {plan['vec_fwd']}/{plan['vec_bwd']}"
    _judge_all(label, ("out", "dqkv", "c2 max", "1 / sum"), (out, dqkv, stat[:, 0], stat[:, 1]), r64, r32, TOLS)

    # the backward alone, on out and rowstat made in float64 and rounded once
    out32, stat32, d64, d32 = sp.backward_ref_on_rounded(c)
    dq2 = _run(lib, dev, qd, dd, S, C, L, out32.to(dev), stat32.to(dev))[3]
    _judge_all(label, ("dqkv (float64-made out, rowstat)",), (dq2,), (d64,), (d32,), (cr.TOL["attn_bwd"],))


def test_stream_refusals_and_empty_calls_write_nothing(dev, lib):
    x = torch.zeros(4096, device=dev)
    outs = [_banded(dev, 4096) for _ in range(4)]
    (o, s, d, g), st = [t for t, _ in outs], _stream()
    buf = (ctypes.c_int * 10)()
    for S, C, L, rc, state in ((2, 0, 16, INVALID, sp.REFUSED), (2, 513, 1, INVALID, sp.REFUSED), (2, -3, 16, INVALID, sp.REFUSED),
                               (0, 64, 16, 0, sp.EMPTY), (2, 64, 0, 0, sp.EMPTY), (-1, 64, 16, 0, sp.EMPTY), (0, 513, 16, 0, sp.EMPTY)):
        assert lib.vf_attn_stream_plan(_P(x), _P(x), S, C, L, ctypes.cast(buf, ctypes.c_void_p)) == 0
        assert list(buf) == sp.plan(0, 0, S, C, L) == [state] + [0] * 9
        assert lib.vf_attn_stream_fwd(_P(x), _P(o), _P(s), S, C, L, st) == rc, (S, C, L)
        assert lib.vf_attn_stream_fwd(_P(x), _P(o), None, S, C, L, st) == rc, (S, C, L)
        assert lib.vf_attn_stream_bwd(_P(x), _P(x), _P(x), _P(x), _P(d), _P(g), S, C, L, st) == rc, (S, C, L)
    assert _intact(*(b for _, b in outs))
    assert all(bool(torch.isnan(t).all()) for t in (o, s, d, g))


# ------------------------------------------------------------------------------------------------ (b) through ops
OPS_SHAPES = [(64, 5, 13, 2), (192, 7, 19, 2), (320, 6, 22, 1), (500, 5, 27, 1)]          # (C, H, W, S): NT = 1, 2, 3, 4


def _through(dev, lib, fn, C, H, W, S, label):
    L = H * W
    qkv = cr.attn_input(S, C, L, 2, 0, sp.SEED)
    dy = cr._u((S, C, L), sp.SEED + 7).float()
    r64, r32 = cr.attn_ref(qkv, dy)
    qg = qkv.reshape(S, 3 * C, H, W).to(dev).requires_grad_(True)
    gy = dy.reshape(S, C, H, W).to(dev)
    with _Log() as names:
        o = fn(qg)
        o.backward(gy)
    with torch.no_grad(), _Log() as names_ng:
        o_ng = fn(qg.detach())
    assert names == ["vf_attn_stream_fwd", "vf_attn_stream_bwd"] and names_ng == ["vf_attn_stream_fwd"], (names, names_ng)
    buf = (ctypes.c_int * 10)()
    assert lib.vf_attn_stream_plan(_P(qg), _P(gy), S, C, L, ctypes.cast(buf, ctypes.c_void_p)) == 0
    plan = dict(zip(sp.FIELDS, buf))
    assert list(buf) == sp.plan(0, 0, S, C, L) and plan["state"] == sp.RUNS and plan["NT"] == sp.tiles_per_wave(C)
    assert torch.equal(o.detach(), o_ng)
    _judge_all(f"{label} ({C},{H}x{W},S={S}) NT {plan['NT']} vec {plan['vec_fwd']}/{plan['vec_bwd']}", ("out", "dqkv"),
               (o.reshape(S, C, -1), qg.grad.reshape(S, 3 * C, -1)), r64, r32, TOLS[:2])
    return plan


@pytest.mark.parametrize("C,H,W,S", OPS_SHAPES, ids=lambda v: str(v))
def test_attention_streaming_through_ops_per_instantiation(dev, lib, C, H, W, S):
    from view_fusion_amd import ops
    _through(dev, lib, ops.attention_streaming, C, H, W, S, "ops.attention_streaming")


@pytest.mark.parametrize("C,H,W,S,vec", [(192, 64, 65, 1, 1), (256, 65, 65, 1, 0)], ids=lambda v: str(v))
def test_the_natural_route_reaches_the_two_tile_instantiations(dev, lib, C, H, W, S, vec):
    """ops.attention above 4096 pixels at 129 <= C <= 256: attn_stream_fwd / dkv / dq_kernel<2>, which SMALL's level-2
    attention (C = 192) takes from a 260 x 260 input on.  S L^2 C = 3.3e9 and 4.6e9: over ATTN_CAP, because the route
    starts at L = 4097."""
    from view_fusion_amd import ops
    assert ops.attention_route(C, H * W) == "stream" and sp.cost(S, C, H * W) > sp.ATTN_CAP
    plan = _through(dev, lib, ops.attention, C, H, W, S, "ops.attention")
    assert (plan["NT"], plan["vec_fwd"], plan["vec_bwd"]) == (2, vec, vec)
