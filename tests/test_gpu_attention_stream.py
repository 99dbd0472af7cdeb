"""ops.attention_streaming (csrc/attention_stream.hip) on a real MI355X: forward and backward against an fp64 closed form
at every C the UNet produces and L on both sides of every tile, O(L) memory, deterministic backward, graph replay."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def reference(qkv, gy, rows=1024):
    """fp64 O and dqkv of softmax(Q^T K / sqrt(C)) V^T, a chunk of query rows at a time (no L x L matrix)."""
    S, C3, H, W = qkv.shape
    C, L = C3 // 3, H * W
    alpha = 1.0 / math.sqrt(C)
    x = qkv.double().reshape(S, 3, C, L)
    dO = gy.double().reshape(S, C, L)
    out, dx = torch.empty(S, C, L, dtype=torch.float64), torch.zeros(S, 3, C, L, dtype=torch.float64)
    for b in range(S):
        q, k, v = x[b]
        for i0 in range(0, L, rows):
            i1 = min(L, i0 + rows)
            p = torch.softmax(alpha * (q[:, i0:i1].T @ k), -1)          # [rows][L]
            o = v @ p.T                                                  # [C][rows]
            out[b, :, i0:i1] = o
            dp = dO[b, :, i0:i1].T @ v                                   # [rows][L]
            ds = p * (dp - (dO[b, :, i0:i1] * o).sum(0)[:, None])
            dx[b, 2] += dO[b, :, i0:i1] @ p
            dx[b, 1] += alpha * q[:, i0:i1] @ ds
            dx[b, 0, :, i0:i1] = alpha * k @ ds.T
    return out.reshape(S, C, H, W), dx.reshape(S, C3, H, W)


CASES = [(8, 6, 10, 3), (48, 10, 10, 17), (64, 16, 16, 3), (128, 36, 36, 3), (320, 64, 64, 1), (64, 66, 66, 3),
         (48, 72, 72, 1), (128, 64, 80, 1), (8, 96, 96, 1), (64, 128, 128, 1), (320, 7, 9, 3), (512, 12, 12, 2)]


@pytest.mark.parametrize("C,H,W,S", CASES, ids=lambda v: str(v))
def test_stream_fwd_bwd_vs_fp64(dev, C, H, W, S):
    from view_fusion_amd import ops
    qkv, gy = rnd(S, 3 * C, H, W, seed=1) * 2, rnd(S, C, H, W, seed=2)
    oc, dc = reference(qkv, gy)
    qg = qkv.to(dev).requires_grad_(True)
    og = ops.attention_streaming(qg)
    og.backward(gy.to(dev))
    assert rel(og, oc) < 2e-5
    assert rel(qg.grad, dc) < 5e-5


def test_stream_memory_is_linear_in_L(dev):
    from view_fusion_amd import ops
    S, C, H = 4, 64, 128
    qkv = (torch.rand(S, 3 * C, H, H, device=dev) * 2 - 1).requires_grad_(True)
    gy = torch.rand(S, C, H, H, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.attention_streaming(qkv)
    out.backward(gy)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    assert grown < 256 * 2 ** 20, grown          # the materialised scores alone: 4 GiB
    assert torch.isfinite(qkv.grad).all()


def test_stream_backward_is_deterministic_and_graph_replay_is_bitwise(dev):
    from view_fusion_amd import ops
    S, C, H, W = 3, 64, 72, 72
    qkv, gy = (rnd(S, 3 * C, H, W, seed=5) * 2).to(dev), rnd(S, C, H, W, seed=6).to(dev)

    def step(x_in, g_in):
        x = x_in.detach().requires_grad_(True)
        o = ops.attention_streaming(x)
        (dx,) = torch.autograd.grad(o, x, g_in)
        return o, dx

    o1, d1 = step(qkv, gy)
    o2, d2 = step(qkv, gy)
    assert torch.equal(o1, o2) and torch.equal(d1, d2)

    sq, sg = qkv.clone(), gy.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                   # one eager warm-up, as train.Trainer._capture
        step(sq, sg)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og, dg = step(sq, sg)
    sq.zero_()
    sg.zero_()
    sq.copy_(qkv)
    sg.copy_(gy)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(og, o1) and torch.equal(dg, d1)


def test_stream_no_grad_matches_grad_call_and_writes_no_lse(dev, monkeypatch):
    from view_fusion_amd import _lib, ops
    S, C, H, W = 2, 48, 66, 66
    qkv = (rnd(S, 3 * C, H, W, seed=7) * 2).to(dev)
    seen = []
    real = _lib.call

    def spy(name, *args):
        if name == "vf_attn_stream_fwd":
            seen.append(args[2])
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    with torch.no_grad():
        oi = ops.attention_streaming(qkv)
    ot = ops.attention_streaming(qkv.clone().requires_grad_(True))
    assert seen[0] is None and seen[1] is not None
    assert oi.grad_fn is None
    assert torch.equal(oi, ot.detach())


def test_attention_routes_large_maps_to_the_streaming_kernels(dev):
    from view_fusion_amd import ops
    qkv, gy = rnd(1, 3 * 32, 72, 72, seed=8) * 2, rnd(1, 32, 72, 72, seed=9)
    qa = qkv.to(dev).requires_grad_(True)
    qb = qkv.to(dev).requires_grad_(True)
    oa, ob = ops.attention(qa), ops.attention_streaming(qb)
    oa.backward(gy.to(dev))
    ob.backward(gy.to(dev))
    assert torch.equal(oa, ob) and torch.equal(qa.grad, qb.grad)
