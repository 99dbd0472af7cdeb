"""Every reachable launch plan of the self-attention block and of the batched GEMM / row softmax beneath it on a real
MI355X against float64 (case lists, class keys and references: tests/attn_plan_ref.py; the plans themselves are pinned to
the library on the CPU in tests/test_attn_plan_host.py).

  (a) every attention case through ops.attention, training (P written) and no-grad (P null): out and d(qkv) against
      cond_ref.attn_ref, the launch list against the plan, vf_attention_fwd_kernel against the class;
  (b) the C ABI alone: vf_attention_fwd with and without P -- the saved P of every forward kernel judged against the
      float64 softmax --, vf_attention_dscore and vf_attention_dvdk each on P and dS computed in float64 and rounded once
      (a wrong P layout is then told from a wrong backward); outputs NaN-filled, a 1024-float band behind each; refusals;
  (c) vf_bgemm on strided views, one case per bgemm class; (d) vf_softmax_fwd / _bwd per softmax class;
  (e) one child process for the routes behind VF_ATTN_Q32=0 VF_ATTN_Q16=0 (read once per process).

One rule (cond_ref.judge): err = max|a - r64| / max|r64|, e = the same for stock fp32 torch on the CPU, pass if
err <= max(4 e, tol), tol = cond_ref.TOL (attn_fwd 2e-5, attn_bwd 5e-5; bgemm: attn_fwd; softmax: four times the largest e
of its case list); a non-finite value fails.  Inputs: cond_ref.attn_input at scale 2, shift 0 -- every view different, so
a permuted view cannot pass.  Measured values: profiles/attn_plan.md."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

import attn_plan_ref as ap
import cond_ref as cr
from test_gpu_conditioning import _Log

pytestmark = pytest.mark.gpu

BAND, SENTINEL = 1024, 12345.0
INVALID = 1                                    # hipErrorInvalidValue


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
        print(f"ATTNPLAN | {label} | {n} | e {e:.3e} | err {d:.3e} | bound {b:.3e} | {'ok' if ok else 'FAIL'}")
    assert all(r[4] for r in rows), [(r[0], r[1], r[3]) for r in rows if not r[4]]


def _P(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _banded(dev, *shape):
    """-> (NaN-filled tensor of `shape`, the sentinel band behind it)."""
    n = math.prod(shape)
    buf = torch.full((n + BAND,), float("nan"), device=dev)
    buf[n:] = SENTINEL
    return buf[:n].view(*shape), buf[n:]


def _intact(*bands):
    torch.cuda.synchronize()
    return all(bool((b == SENTINEL).all()) for b in bands)


# ------------------------------------------------------------------------------------------------ (a) through ops
@pytest.mark.parametrize("c", ap.attention_cases(), ids=ap.a_id)
def test_attention_plan_through_ops(dev, lib, c):
    from view_fusion_amd import ops
    S, C, L = c.S, c.C, c.H * c.W
    fwd, plan = ap.fwd_key(S, C, L), ap.bwd_plan(S, C, L, c.dscore, c.dvdk)
    assert ap.KERNEL_NAMES[lib.vf_attention_fwd_kernel(S, C, L) if L in (64, 256) else 0] == fwd[1]
    assert ops.attention_route(C, L) == ("generic" if fwd[1] == "generic" else "fused")
    qkv, dy = ap.attn_tensors(c)
    r64, r32 = cr.attn_ref(qkv, dy)
    qg = qkv.reshape(S, 3 * C, c.H, c.W).to(dev).requires_grad_(True)
    old = (ops.st.ATTN_DSCORE, ops.st.ATTN_DVDK)
    try:
        ops.st.ATTN_DSCORE, ops.st.ATTN_DVDK = bool(c.dscore), bool(c.dvdk)
        with _Log() as names:
            o = ops.attention(qg)
            o.backward(dy.reshape(S, C, c.H, c.W).to(dev))
        with torch.no_grad(), _Log() as names_ng:
            o_ng = ops.attention(qg.detach())
    finally:
        ops.st.ATTN_DSCORE, ops.st.ATTN_DVDK = old
    assert names == ap.fwd_launches(C, L) + ap.bwd_launches(plan), names
    assert names_ng == ap.fwd_launches(C, L), names_ng
    _judge_all(f"ops {ap.a_id(c)} {fwd[1]} / {ap.bwd_key(S, C, L, c.dscore, c.dvdk)[2]}", ("out", "dqkv", "out (no-grad)"),
               (o.reshape(S, C, -1), qg.grad.reshape(S, 3 * C, -1), o_ng.reshape(S, C, -1)), (r64[0], r64[1], r64[0]),
               (r32[0], r32[1], r32[0]), (cr.TOL["attn_fwd"], cr.TOL["attn_bwd"], cr.TOL["attn_fwd"]))


# ------------------------------------------------------------------------------------------------ (b) the C ABI alone
# one shape per (forward kernel, L, placement class): (S, C, L)
FWD_ABI = [(1, 64, 256), (3, 128, 256), (16, 64, 256), (3, 32, 256), (8, 96, 256), (11, 32, 256), (19, 64, 256), (97, 32, 256),
           (1, 64, 64), (5, 128, 64), (1, 32, 64), (3, 96, 64), (17, 64, 64)]
DSCORE_ABI = [(S, C) for S in (3, 8, 11) for C in (32, 64, 96)]
DVDK_ABI = [(S, C) for S in (1, 2, 3, 4, 5, 6, 7, 8, 11) for C in (64, 192)]


def _softmax32(qkv):
    S, C3, L = qkv.shape
    q, k, _ = qkv.reshape(S, 3, C3 // 3, L).unbind(1)
    return torch.softmax(torch.bmm(q.transpose(1, 2), k) / math.sqrt(C3 // 3), -1)


@pytest.mark.parametrize("S,C,L", FWD_ABI)
def test_forward_abi_writes_out_and_the_probabilities(dev, lib, S, C, L):
    """vf_attention_fwd with P given and with P null: out both times, and the P each forward kernel saves, row-major
    [view][query][key] as the backward reads it."""
    qkv = cr.attn_input(S, C, L, 2, 0, ap.SEED)
    o64, p64 = cr.attn_forward_f64(qkv)
    p32 = _softmax32(qkv)
    o32 = torch.bmm(qkv.reshape(S, 3, C, L)[:, 2], p32.transpose(1, 2))
    qd = qkv.to(dev)
    out, b0 = _banded(dev, S, C, L)
    P, b1 = _banded(dev, S, L, L)
    out2, b2 = _banded(dev, S, C, L)
    assert lib.vf_attention_fwd(_P(qd), _P(out), _P(P), S, C, L, _stream()) == 0
    assert lib.vf_attention_fwd(_P(qd), _P(out2), None, S, C, L, _stream()) == 0
    assert _intact(b0, b1, b2)
    kernel = ap.KERNEL_NAMES[lib.vf_attention_fwd_kernel(S, C, L)]
    _judge_all(f"abi fwd {kernel} S{S} C{C} L{L}", ("out", "P", "out (P null)"), (out, P, out2), (o64, p64, o64), (o32, p32, o32),
               (cr.TOL["attn_fwd"],) * 3)


def _bwd_inputs(S, C, L):
    """-> qkv, dO, P, dS (float32; P and dS computed in float64 and rounded once) and the float64 / fp32 [dS, dq, dk, dv]
    of the backward on exactly those rounded P (and, for dk, dS)."""
    qkv = cr.attn_input(S, C, L, 2, 0, ap.SEED)
    dO = cr._u((S, C, L), ap.SEED + 7).float()
    P = cr.attn_forward_f64(qkv)[1].float()

    def run(dt, dS_in=None):
        q, k, v = qkv.to(dt).reshape(S, 3, C, L).unbind(1)
        p, a = P.to(dt), 1.0 / math.sqrt(C)
        dp = torch.bmm(dO.to(dt).transpose(1, 2), v)
        ds = p * (dp - (p * dp).sum(-1, keepdim=True))
        dsk = ds if dS_in is None else dS_in.to(dt)
        return [ds, a * torch.bmm(k, ds.transpose(1, 2)), a * torch.bmm(q, dsk), torch.bmm(dO.to(dt), p)]
    dS = run(torch.float64)[0].float()
    return qkv, dO, P, dS, run(torch.float64, dS), run(torch.float32, dS)


@pytest.mark.parametrize("S,C", DSCORE_ABI)
def test_dscore_abi_alone(dev, lib, S, C):
    L = 256
    qkv, dO, P, _, r64, r32 = _bwd_inputs(S, C, L)
    dS, b0 = _banded(dev, S, L, L)
    dqkv, b1 = _banded(dev, S, 3, C, L)
    assert lib.vf_attention_dscore(_P(qkv.to(dev)), _P(dO.to(dev)), _P(P.to(dev)), _P(dS), _P(dqkv), S, C, L, _stream()) == 0
    assert _intact(b0, b1)
    assert bool(torch.isnan(dqkv[:, 1:]).all()), "the k and v thirds belong to the other launch"
    _judge_all(f"abi dscore S{S} C{C}", ("dS", "dq"), (dS, dqkv[:, 0]), r64[:2], r32[:2], (cr.TOL["attn_bwd"],) * 2)


@pytest.mark.parametrize("S,C", DVDK_ABI)
def test_dvdk_abi_alone(dev, lib, S, C):
    L = 256
    qkv, dO, P, dS, r64, r32 = _bwd_inputs(S, C, L)
    dqkv, b0 = _banded(dev, S, 3, C, L)
    assert lib.vf_attention_dvdk(_P(qkv.to(dev)), _P(dO.to(dev)), _P(P.to(dev)), _P(dS.to(dev)), _P(dqkv), S, C, L, _stream()) == 0
    assert _intact(b0)
    assert bool(torch.isnan(dqkv[:, 0]).all()), "the q third belongs to the other launch"
    _judge_all(f"abi dvdk S{S} C{C}", ("dk", "dv"), (dqkv[:, 1], dqkv[:, 2]), r64[2:], r32[2:], (cr.TOL["attn_bwd"],) * 2)


def test_attention_refusals_write_nothing(dev, lib):
    S, L = 2, 256
    x = torch.zeros(S * 3 * 96 * L, device=dev)
    outs = [_banded(dev, S * 3 * 96 * L)[0] for _ in range(3)]
    st = _stream()
    assert lib.vf_attention_fwd(_P(x), _P(outs[0]), _P(outs[1]), S, 48, 256, st) == INVALID      # C % 32 != 0
    assert lib.vf_attention_fwd(_P(x), _P(outs[0]), _P(outs[1]), S, 48, 64, st) == INVALID
    for bad_L in (128, 60, 1024):                                                               # L not in {64, 256}
        assert lib.vf_attention_fwd(_P(x), _P(outs[0]), _P(outs[1]), S, 32, bad_L, st) == INVALID
        assert lib.vf_attention_fwd_kernel(S, 32, bad_L) == 0
    assert lib.vf_attention_dscore(_P(x), _P(x), _P(x), _P(outs[0]), _P(outs[1]), S, 64, 64, st) == INVALID      # dscore at L = 64
    assert lib.vf_attention_dscore(_P(x), _P(x), _P(x), _P(outs[0]), _P(outs[1]), S, 48, 256, st) == INVALID
    assert lib.vf_attention_dvdk(_P(x), _P(x), _P(x), _P(x), _P(outs[2]), S, 96, 256, st) == INVALID             # dvdk at C = 96
    assert lib.vf_attention_dvdk(_P(x), _P(x), _P(x), _P(x), _P(outs[2]), S, 64, 64, st) == INVALID
    for S0 in (0, -1):                                                                         # no views: success, nothing runs
        assert lib.vf_attention_fwd(_P(x), _P(outs[0]), _P(outs[1]), S0, 64, 256, st) == 0
        assert lib.vf_attention_dscore(_P(x), _P(x), _P(x), _P(outs[0]), _P(outs[1]), S0, 64, 256, st) == 0
        assert lib.vf_attention_dvdk(_P(x), _P(x), _P(x), _P(x), _P(outs[2]), S0, 64, 256, st) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)


# ------------------------------------------------------------------------------------------------ (c) vf_bgemm
@pytest.mark.parametrize("c", ap.bgemm_cases(), ids=ap.b_id)
def test_bgemm_plan_class(dev, lib, c):
    """One case per bgemm class on strided views of larger buffers (offsets included): the contraction against float64,
    beta on a pre-filled C, bias along n, nothing written outside the view, run 2 = run 1 bit for bit."""
    A, B, C0, bias = ap.b_tensors(c)
    plan = ap.b_plan(c)
    buf, p = (ctypes.c_int * 7)(), None
    Ad, Bd, bd = A.to(dev), B.to(dev), bias.to(dev) if bias is not None else None
    assert lib.vf_bgemm_plan(_P(Ad, c.offA), _P(Bd, c.offB), c.batch, c.M, c.N, c.K, *c.sA, *c.sB, c.sC[2],
                             ctypes.cast(buf, ctypes.c_void_p)) == 0
    assert list(buf) == plan, (list(buf), plan)          # (on the real addresses: torch's allocations are 16-byte aligned)
    idx = ap.b_index(c.offC, c.sC, (c.batch, c.M, c.N))
    assert idx.unique().numel() == idx.numel() and int(idx.max()) < C0.numel()
    if c.beta == 0:
        C0 = C0.clone()
        C0[idx] = float("nan")                           # beta = 0 may not read C
    runs = []
    for _ in range(2):
        Cd = torch.cat([C0, torch.full((BAND,), SENTINEL)]).to(dev)
        assert lib.vf_bgemm(_P(Ad, c.offA), _P(Bd, c.offB), _P(Cd, c.offC), _P(bd), c.batch, c.M, c.N, c.K, *c.sA, *c.sB, *c.sC,
                            c.alpha, c.beta, _stream()) == 0
        torch.cuda.synchronize()
        runs.append(Cd.cpu())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "run 2 differs from run 1"
    got = runs[0][idx]
    rest, rest0 = runs[0].clone(), torch.cat([C0, torch.full((BAND,), SENTINEL)])
    rest[idx], rest0[idx] = 0.0, 0.0
    assert torch.equal(rest, rest0), "written outside the view"
    r64, r32 = ap.b_ref(c, A, B, C0, bias, torch.float64), ap.b_ref(c, A, B, C0, bias, torch.float32)
    _judge_all(f"bgemm {ap.b_id(c)} {' | '.join(str(v) for v in ap.b_key(c)[1:])}", ("C",), (got,), (r64,), (r32,), (cr.TOL["attn_fwd"],))


def test_bgemm_empty_products_launch_nothing(dev, lib):
    x = torch.zeros(64, device=dev)
    out = _banded(dev, 64)[0]
    for batch, M, N in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (-1, 4, 4)):
        assert lib.vf_bgemm(_P(x), _P(x), _P(out), None, batch, M, N, 4, 16, 4, 1, 16, 4, 1, 16, 4, 1, 1.0, 0.0, _stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ (d) the row softmax
@pytest.mark.parametrize("rows,cols", ap.softmax_cases())
def test_softmax_plan_class(dev, lib, rows, cols):
    """vf_softmax_fwd and vf_softmax_bwd per (MAXV, cols on an edge | ragged against 64, rows % 4), out of place into
    NaN-filled banded outputs and in place as ops.attention calls them (y over x; dx over dy): the same bits."""
    x, y, dy = ap.softmax_tensors(rows, cols)
    r64, r32 = ap.softmax_refs(x, y, dy)
    buf = (ctypes.c_int * 2)()
    assert lib.vf_softmax_plan(rows, cols, ctypes.cast(buf, ctypes.c_void_p)) == 0 and list(buf) == ap.softmax_plan(rows, cols)
    xd, yd, dyd = x.to(dev), y.to(dev), dy.to(dev)
    out, b0 = _banded(dev, rows, cols)
    dx, b1 = _banded(dev, rows, cols)
    assert lib.vf_softmax_fwd(_P(xd), _P(out), rows, cols, _stream()) == 0
    assert lib.vf_softmax_bwd(_P(yd), _P(dyd), _P(dx), rows, cols, _stream()) == 0
    assert _intact(b0, b1)
    xi, dyi = xd.clone(), dyd.clone()
    assert lib.vf_softmax_fwd(_P(xi), _P(xi), rows, cols, _stream()) == 0
    assert lib.vf_softmax_bwd(_P(yd), _P(dyi), _P(dyi), rows, cols, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(xi, out) and torch.equal(dyi, dx)
    _judge_all(f"softmax MAXV {buf[0]} rows {rows} cols {cols}", ("y", "dx"), (out, dx), r64, r32, (cr.TOL["softmax"],) * 2)


def test_softmax_refusals_write_nothing(dev, lib):
    x = torch.zeros(4 * 4100, device=dev)
    out = _banded(dev, 4 * 4100)[0]
    for cols in (4097, 4100, 8192):
        assert lib.vf_softmax_fwd(_P(x), _P(out), 4, cols, _stream()) == INVALID
        assert lib.vf_softmax_bwd(_P(x), _P(x), _P(out), 4, cols, _stream()) == INVALID
    for rows in (0, -3):
        assert lib.vf_softmax_fwd(_P(x), _P(out), rows, 64, _stream()) == 0
        assert lib.vf_softmax_bwd(_P(x), _P(x), _P(out), rows, 64, _stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ (e) the tuning-aid routes
def test_tuning_aid_routes_in_a_fresh_process():
    """VF_ATTN_Q32=0 VF_ATTN_Q16=0 (the round-4 choice; read once per process, hence the child): attn_fwd_split_kernel<256>
    at S = 3, the S = 52 / 53 hand-over to the 128-query kernel, the key-split kernel at L = 64; tests/attn_plan_child.py
    runs them one after the other, judges them by the same rule and exits non-zero on the first failure."""
    env = dict(os.environ, VF_ATTN_Q32="0", VF_ATTN_Q16="0")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_plan_child.py")
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=240)
    print()
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count("ATTNPLAN | child") == 8 and "FAIL" not in r.stdout
