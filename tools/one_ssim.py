#!/usr/bin/env python3
"""Time ops.ssim at one shape, after warm-up, next to what a user had to do without it: the same formula as torch
grouped convolutions on the GPU, passed to drivers.evaluate through extra_metrics.

    python tools/one_ssim.py B C H W [--seconds S] [--no-torch]

Prints one line per path: mean ms per call over back-to-back calls between two HIP events (the repetition count is
chosen so that the timed window lasts about S seconds), the launches per call where the path counts them, and the
achieved bytes per second on the algorithmic traffic 2 B C H W 4 (both images read once) with its share of the 8 TB/s
HBM peak.  `ops.ssim (graph)` replays a captured call: device time without the host's enqueue cost.  The line
`max |ours - torch|` compares the two results on the timed inputs.  For kernel times run it under
`rocprofv3 --kernel-trace --stats -- python tools/one_ssim.py ...`."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from view_fusion_amd import _lib, ops  # noqa: E402

HBM_PEAK = 8.0e12


def torch_ssim(X, Y, data_range=1.0):
    """pytorch_msssim.ssim(X, Y, data_range, size_average=False) with its defaults, as stock torch ops."""
    C = X.shape[1]
    win = ops.diffusion._ssim_window(X.device).reshape(1, 1, 1, -1).repeat(C, 1, 1, 1)

    def filt(t):
        t = F.conv2d(t, win.transpose(2, -1), groups=C)
        return F.conv2d(t, win, groups=C)

    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = filt(X), filt(Y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq, sigma2_sq, sigma12 = filt(X * X) - mu1_sq, filt(Y * Y) - mu2_sq, filt(X * Y) - mu1_mu2
    cs_map = (2 * sigma12 + C2) / (sigma1_sq + sigma2_sq + C2)
    ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return torch.flatten(ssim_map, 2).mean(-1).mean(1)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fn, seconds):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    reps = max(50, int(seconds * 1e3 / max(window(fn, 50), 1e-4)))
    return window(fn, reps), reps


def report(name, ms, reps, nbytes, launches=None):
    rate = nbytes / (ms * 1e-3)
    extra = "" if launches is None else f"  {launches} launches"
    print(f"{name:18s} {ms * 1e3:9.2f} us/call over {reps:6d} calls  {rate / 1e9:8.1f} GB/s  "
          f"{rate / HBM_PEAK:6.4f} of HBM peak{extra}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("B", type=int)
    ap.add_argument("C", type=int)
    ap.add_argument("H", type=int)
    ap.add_argument("W", type=int)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    Y = torch.rand(a.B, a.C, a.H, a.W, generator=g)
    X = (Y + 0.05 * torch.randn(a.B, a.C, a.H, a.W, generator=g)).clamp(0, 1)
    X, Y = X.cuda(), Y.cuda()
    nbytes = 2.0 * X.numel() * 4
    print(f"B={a.B} C={a.C} H={a.H} W={a.W}  algorithmic bytes {nbytes / 1e6:.2f} MB", flush=True)

    n0 = _lib.N_CALLS
    ours = ops.ssim(X, Y)
    entries = _lib.N_CALLS - n0
    ms, reps = timed(lambda: ops.ssim(X, Y), a.seconds)
    report("ops.ssim", ms, reps, nbytes, launches=2 * entries)          # vf_ssim: the tile kernel + the finish kernel

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.ssim(X, Y)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ops.ssim(X, Y)
    ms, reps = timed(graph.replay, a.seconds)
    report("ops.ssim (graph)", ms, reps, nbytes)

    if not a.no_torch:
        with torch.no_grad():
            ref = torch_ssim(X, Y)
            ms, reps = timed(lambda: torch_ssim(X, Y), a.seconds)
        report("torch grouped conv", ms, reps, nbytes)
        print(f"max |ours - torch| {float((ours - ref).abs().max()):.3e}", flush=True)


if __name__ == "__main__":
    main()
