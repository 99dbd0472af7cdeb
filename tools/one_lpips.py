#!/usr/bin/env python3
"""Time ops.lpips at one shape, after warm-up, next to the same metric as stock torch ops on the GPU (the lpips
package's operation order: what a user runs without ops.lpips; the ATen launches are the package's).  The network has
the real VGG16 widths and seeded synthetic weights -- time does not depend on the values.

    python tools/one_lpips.py B H W [--seconds S] [--only ours|torch] [--calls N]

Prints the conv route ops.conv2d takes for each of the 13 layers, then one line per path: mean ms per call over
back-to-back calls between two HIP events, and for ours the C-ABI entries per call (a conv entry is one kernel, two
where it runs split-K or has Winograd tail tiles).  `ops.lpips (graph)` replays a captured call.  For kernel counts
and times run one path alone for a fixed number of calls under the profiler:
`rocprofv3 --kernel-trace --stats -- python tools/one_lpips.py 16 64 64 --only ours --calls 20`."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from view_fusion_amd import _lib, drivers, ops  # noqa: E402

GROUPS = (2, 2, 3, 3, 3)


def synthetic_net(dev):
    g = torch.Generator().manual_seed(0)
    net = drivers.LPIPS()
    for conv in net.convs:
        fan_in = conv.weight.shape[1] * 9
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
        conv.bias.copy_((torch.rand(conv.bias.shape, generator=g) - 0.5) * 0.2)
    for lin in net.lins:
        lin.copy_(torch.rand(lin.shape, generator=g) / lin.shape[1])
    return net.to(dev)


def torch_lpips(X, Y, net):
    shift = torch.tensor([-.030, -.088, -.188], device=X.device).reshape(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], device=X.device).reshape(1, 3, 1, 1)

    def taps(x):
        h, out, it = (2 * x - 1 - shift) / scale, [], iter(net.convs)
        for gi, n in enumerate(GROUPS):
            if gi:
                h = F.max_pool2d(h, 2, 2)
            for _ in range(n):
                c = next(it)
                h = F.relu(F.conv2d(h, c.weight, c.bias, padding=1))
            out.append(h)
        return out

    val = 0
    for a, b, w in zip(taps(X), taps(Y), net.lins):
        na = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + 1e-10)
        nb = b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + 1e-10)
        val = val + F.conv2d((na - nb) ** 2, w).mean([2, 3], keepdim=True)
    return val.reshape(-1)


def routes(S, H, W, net):
    lib = _lib.load()
    names = {0: "direct", 1: "nested Winograd", 2: "Winograd F(4x4)"}
    it = iter(net.convs)
    for gi, n in enumerate(GROUPS):
        h, w = H >> gi, W >> gi
        for _ in range(n):
            c = next(it)
            co, ci = c.weight.shape[0], c.weight.shape[1]
            kind = ops.wino_kind(S, ci, co, h, w, 3, 0, train=False)
            note = ""
            if kind == 0:
                pow2 = h == w and h in (8, 16, 32, 64, 128)
                note = " (specialised)" if pow2 else " (any-size kernel)"
                if lib.vf_conv_fwd_ws_floats(S, ci, co, h, w, 3) > 0:
                    note += " + split-K reduce"
            print(f"  conv {ci:3d} -> {co:3d} at {h:3d}x{w:<3d} S={S}: {names[kind]}{note}", flush=True)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fn, seconds):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    reps = max(10, int(seconds * 1e3 / max(window(fn, 10), 1e-4)))
    return window(fn, reps), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("B", type=int)
    ap.add_argument("H", type=int)
    ap.add_argument("W", type=int)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--only", choices=["ours", "torch"])
    ap.add_argument("--calls", type=int, default=0, help="with --only: run exactly N calls after one warm-up, no timing")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    Y = torch.rand(a.B, 3, a.H, a.W, generator=g)
    X = (Y + 0.05 * torch.randn(a.B, 3, a.H, a.W, generator=g)).clamp(0, 1)
    X, Y = X.to(dev), Y.to(dev)
    with torch.no_grad():
        net = synthetic_net(dev)
    ours_fn = lambda: ops.lpips(X, Y, net)
    torch_fn = lambda: torch_lpips(X, Y, net)
    if a.only and a.calls:
        fn = ours_fn if a.only == "ours" else torch_fn
        with torch.no_grad():
            fn()
            torch.cuda.synchronize()
            for _ in range(a.calls):
                fn()
        torch.cuda.synchronize()
        print(f"{a.only}: {a.calls} calls after one warm-up call", flush=True)
        return
    print(f"B={a.B} H={a.H} W={a.W}", flush=True)
    ours = ref = None
    if a.only != "torch":
        routes(2 * a.B, a.H, a.W, net)
        ours = ours_fn()                                   # packs the weights
        n0 = _lib.N_CALLS
        ours = ours_fn()
        entries = _lib.N_CALLS - n0
        ms, reps = timed(ours_fn, a.seconds)
        print(f"ops.lpips          {ms * 1e3:9.1f} us/call over {reps:5d} calls  {entries} C-ABI entries", flush=True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ours_fn()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ours_fn()
        ms, reps = timed(graph.replay, a.seconds)
        print(f"ops.lpips (graph)  {ms * 1e3:9.1f} us/call over {reps:5d} calls", flush=True)
    if a.only != "ours":
        with torch.no_grad():
            ref = torch_fn()
            ms, reps = timed(torch_fn, a.seconds)
        print(f"torch ops          {ms * 1e3:9.1f} us/call over {reps:5d} calls", flush=True)
    if ours is not None and ref is not None:
        print(f"max |ours - torch| {float((ours - ref).abs().max()):.3e}  (values about {float(ref.mean()):.3e})", flush=True)


if __name__ == "__main__":
    main()
