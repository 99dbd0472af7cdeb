#!/usr/bin/env python3
"""Time the streaming attention (ops.attention_streaming) forward and backward at one shape, after warm-up, and the
materialised path (ops.attention) next to it where L <= 4096.

    python tools/one_attn_stream.py S C H W [--reps N] [--no-generic]

Prints one line per (path, pass): mean ms per call over N back-to-back calls between two events, and the share of the
157.3 TF fp32 MFMA peak on executed FLOPs (forward 4 S L^2 C, streaming backward 14 S L^2 C, materialised backward
8 S L^2 C).  For kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/one_attn_stream.py ...`."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from view_fusion_amd import ops  # noqa: E402

PEAK = 157.3e12


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(name, op, S, C, H, W, reps, bwd_flops):
    L = H * W
    qkv = (torch.rand(S, 3 * C, H, W, device="cuda") * 2 - 1).requires_grad_(True)
    gy = torch.rand(S, C, H, W, device="cuda") * 2 - 1
    with torch.no_grad():
        tf = timed(lambda: op(qkv), reps)
    out = op(qkv)

    def bwd():
        torch.autograd.grad(out, qkv, gy, retain_graph=True)
    tb = timed(bwd, reps)
    for tag, ms, fl in (("fwd", tf, 4.0 * S * L * L * C), ("bwd", tb, bwd_flops * S * L * L * C)):
        print(f"{name:9s} {tag} S={S:3d} C={C:3d} L={L:6d}  {ms:9.3f} ms  {fl / ms / 1e9:7.1f} TF  "
              f"{fl / ms / 1e-3 / PEAK:5.3f} of peak", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("S", type=int)
    ap.add_argument("C", type=int)
    ap.add_argument("H", type=int)
    ap.add_argument("W", type=int)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-generic", action="store_true")
    a = ap.parse_args()
    run("stream", ops.attention_streaming, a.S, a.C, a.H, a.W, a.reps, 14.0)
    if a.H * a.W <= 4096 and not a.no_generic:
        run("generic", ops.attention, a.S, a.C, a.H, a.W, a.reps, 8.0)


if __name__ == "__main__":
    main()
