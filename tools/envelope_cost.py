"""Cost of the general-geometry path (profiles/r07_envelope_cost.md): SMALL-config train iteration (fwd + bwd,
eager launches) at 48x64 vs 64x64, B = 16, N = 6; B = 1 sampler reverse step at N = 1 / 6; per-layer general 3x3 conv
forward time and fraction of the fp32 MFMA peak on executed FLOPs.

    python tools/envelope_cost.py [OUT.json]          # all legs, JSON to stdout (and OUT.json)
    python tools/envelope_cost.py --train48 N         # only N timed 48x64 train iterations (for a rocprofv3 run)
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from view_fusion_amd import UNet, ViewFusion, ops  # noqa: E402
from view_fusion_amd.utils import deterministic_fill_  # noqa: E402

SMALL = dict(in_channel=6, out_channel=6, inner_channel=64, norm_groups=32, channel_mults=(1, 2, 3, 5), attn_res=(16,),
             res_blocks=3, image_size=64)
SCHED = dict(schedule="linear", num_timesteps=2000, linear_start=1e-6, linear_end=1e-2)
dev = torch.device("cuda:0")
out = {}


def timed(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


train48 = int(sys.argv[sys.argv.index("--train48") + 1]) if "--train48" in sys.argv else 0
net = UNet(**SMALL)
deterministic_fill_(net.state_dict())
vf = ViewFusion(net, {"train": SCHED}, True, True).to(dev)
vf.set_new_noise_schedule(device=dev, phase="train")
for H, W in (((48, 64),) if train48 else ((64, 64), (48, 64))):
    B, N = 16, 6
    g = torch.Generator().manual_seed(0)
    y0, yc = torch.rand(B, 3, H, W, generator=g).to(dev), torch.rand(B, N, 3, H, W, generator=g).to(dev)
    ang = (2 * np.pi / 24 * torch.randint(0, 24, (B, 1), generator=g).float()).to(dev)
    vc = torch.full((B,), N)

    def step():
        vf.zero_grad(set_to_none=True)
        vf(y_cond=yc, view_count=vc, angle=ang, y_0=y0).backward()
    out[f"train_fwd_bwd_ms_{H}x{W}"] = timed(step, train48 or 10)
if train48:
    print(json.dumps(out))
    sys.exit(0)
out["train_per_pixel_ratio_48x64_vs_64x64"] = (out["train_fwd_bwd_ms_48x64"] / (48 * 64)) / (out["train_fwd_bwd_ms_64x64"] / 4096)

for N in (1, 6):
    H, W = 48, 64
    g = torch.Generator().manual_seed(1)
    yt, yc = torch.rand(1, 3, H, W, generator=g).to(dev), torch.rand(1, N, 3, H, W, generator=g).to(dev)
    ang = torch.zeros(1, 1, device=dev)
    t = torch.tensor([500], device=dev)

    def rs():
        with torch.no_grad():
            vf.p_sample(yt, yc, torch.tensor([N]), ang, t)
    out[f"sampler_step_ms_48x64_N{N}_eager"] = timed(rs, 20)

# per-layer: the 3x3 stride-1 layers of SMALL at 48x64, S = 96, forward through the general kernel
layers = {}
for (cin, cout, H, W) in ((64, 64, 48, 64), (128, 128, 24, 32), (192, 192, 12, 16), (320, 320, 6, 8)):
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1).to(dev)
    x = torch.randn(96, cin, H, W, device=dev)
    with torch.no_grad():
        ms = timed(lambda: ops.conv2d(x, conv), 20)
    fl = 2.0 * 96 * cout * cin * 9 * H * W
    layers[f"{cin}->{cout}@{H}x{W}"] = dict(ms=ms, frac_of_157TF=fl / (ms * 1e-3) / 157.3e12)
    xg = x.clone().requires_grad_(True)
    conv.weight.requires_grad_(True)

    def fb():
        y = ops.conv2d(xg, conv)
        y.backward(torch.ones_like(y))
    ms3 = timed(fb, 10)
    layers[f"{cin}->{cout}@{H}x{W}"].update(fwd_dgrad_wgrad_ms=ms3, frac3=3 * fl / (ms3 * 1e-3) / 157.3e12)
out["conv3x3_s96"] = layers
if len(sys.argv) > 1 and sys.argv[1].endswith(".json"):
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
