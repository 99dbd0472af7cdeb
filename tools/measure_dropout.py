"""Measurements behind profiles/dropout_seeded.md (one process per flavour, one GPU, small UNet 64x64).

  python tools/measure_dropout.py step [--dropout P] [--unseeded] [--tag NAME]
      one replayed C2 training step (B = 16, N = 6, S = 96) of a UNet(dropout=P) model under Trainer(graph=True): 4 warm
      steps (two eager, the capture, a replay), then 6 rounds of 20 replays; prints one JSON line with the per-round
      ms / step (median, min, max) and torch.cuda.max_memory_allocated.  Default: Trainer(seed=0) -- the seeded masks
      on a tree that has them, torch's generator on one from before; --unseeded: Trainer(seed=None).  Uses nothing newer
      than UNet(dropout=) and Trainer(seed=), so the same file runs on the parent commit's tree: run the flavours as
      alternating processes (parent, seeded, unseeded, parent, ...) and read the process-to-process spread off the
      repeats.
  python tools/measure_dropout.py layers
      the Dropout inputs of that step by layer, and their summed size (what the unseeded path saves as u), no GPU.
  python tools/measure_dropout.py kernel
      the Dropout launches alone on the step's four layer shapes: rand_like + vf_dropout against vf_dropout_seeded, the
      backward launches likewise; HIP events around 20 back-to-back launches, median of 5 rounds, with the algorithmic
      GB/s of each.
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from view_fusion_amd import train  # noqa: E402

B, N, HW = 16, 6, 64
med = lambda v: sorted(v)[len(v) // 2]


def layer_shapes(net, H, W):
    """(C, H, W) of the activation each residual block's Dropout sees, in execution order."""
    out = []
    for m in list(net.downs) + list(net.mid) + list(net.ups):
        if hasattr(m, "res_block"):
            conv = m.res_block.block2["block"]["3"]
            lvl = conv._vf_geom[0]
            out.append((conv.weight.shape[1], H >> lvl, W >> lvl))
    return out


def layers():
    from view_fusion_amd import UNet
    shapes = layer_shapes(UNet(**dict(train.SMALL_UNET, dropout=0.1)), HW, HW)
    S, per_view = B * N, sum(c * h * w for c, h, w in shapes)
    for i, (c, h, w) in enumerate(shapes):
        print(f"layer {i:2d}: {c:3d} x {h:2d} x {w:2d}  {S * c * h * w * 4 / 2 ** 20:7.2f} MiB at S = {S}")
    print(json.dumps(dict(layers=len(shapes), elements_per_view=per_view, S=S, dropout_input_bytes=S * per_view * 4)))


def step(p, seeded, tag):
    dev = torch.device("cuda:0")
    batch = train.synthetic_batch(B, N, HW, dev, seed=0)
    m = train.build_model(unet_params=dict(train.SMALL_UNET, dropout=p), device="cuda:0", seed=0)
    tr = train.Trainer(m, graph=True, seed=0 if seeded else None)
    torch.cuda.reset_peak_memory_stats()
    for _ in range(4):
        tr.step(batch)
    torch.cuda.synchronize()
    rounds = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            loss = tr.step(batch)
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) / 20 * 1e3)
    assert bool(torch.isfinite(loss))
    print(json.dumps(dict(tag=tag, dropout=p, seeded=seeded, mode=tr.mode, graph_steps=tr.graph_steps,
                          ms_per_step=dict(median=round(med(rounds), 4), min=round(min(rounds), 4), max=round(max(rounds), 4)),
                          max_memory_allocated=torch.cuda.max_memory_allocated())), flush=True)


def kernel():
    from view_fusion_amd import ops
    dev = torch.device("cuda:0")
    S, p = B * N, 0.1
    ids = torch.arange(B, dtype=torch.int64, device=dev)
    off, _, _ = ops.view_offsets([N] * B, dev)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / 20 * 1e3)
        return med(out)

    res = {}
    for c, hw in ((64, 64), (128, 32), (192, 16), (320, 8)):
        x = torch.randn(S, c, hw, hw, device=dev)
        u = torch.rand_like(x)
        nb = x.numel() * 4
        with torch.no_grad():
            row = dict(fwd_unseeded_us=timed(lambda: ops.dropout(x, p)),                 # rand_like + vf_dropout: 16 B / element
                       bwd_unseeded_us=timed(lambda: ops.dropout(x, p, u=u)),            # vf_dropout on (dy, u): 12 B / element
                       seeded_us=timed(lambda: ops.dropout_seeded(x, p, 0, ids, off, 3)))    # either direction: 8 B / element
        row.update(fwd_unseeded_GBps=round(4 * nb / row["fwd_unseeded_us"] / 1e3, 1),
                   bwd_unseeded_GBps=round(3 * nb / row["bwd_unseeded_us"] / 1e3, 1),
                   seeded_GBps=round(2 * nb / row["seeded_us"] / 1e3, 1))
        res[f"{c}x{hw}x{hw}"] = {k: round(v, 2) for k, v in row.items()}
        print(f"{c:3d} x {hw}^2 at S = {S}: " + "  ".join(f"{k} {v:.2f}" for k, v in row.items()), flush=True)
    print(json.dumps({"dropout_kernels": res}), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "layers":
        layers()
    elif sys.argv[1] == "kernel":
        kernel()
    else:
        a = sys.argv[2:]
        p = float(a[a.index("--dropout") + 1]) if "--dropout" in a else 0.1
        step(p, "--unseeded" not in a, a[a.index("--tag") + 1] if "--tag" in a else "")
