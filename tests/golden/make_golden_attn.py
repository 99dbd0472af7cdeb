#!/usr/bin/env python3
"""Golden vectors for attention maps above 4096 pixels, from the REAL reference (see make_golden.py for how the
reference is reached; run in the build container only):

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_attn.py

  envelope_attn_72x72.npz
        ATTN0 (attention on level 0, 72x72 = 5184 pixels; the mid block's attention on 36x36) at S = 2.  Only the seed of
        the inputs is stored (x, angle, level and the output cotangent gy are drawn from it in this order), with digests
        of the UNet output, of the input gradient and of every parameter gradient, the reference run in fp64.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import UNet, deterministic_fill_, grads_digest, tensor_digest  # noqa: E402

ATTN0 = dict(in_channel=6, out_channel=6, inner_channel=32, norm_groups=32, channel_mults=(1, 2), attn_res=(16,),
             res_blocks=1, image_size=16)


def inputs(seed, S, H, W):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(S, 6, H, W, generator=g)
    angle = 2 * np.pi / 24 * torch.randint(0, 24, (S, 1), generator=g).float()
    level = torch.rand(S, 1, generator=g)
    gy = torch.randn(S, 6, H, W, generator=g)
    return x, angle, level, gy


def digest(prefix, t):
    d = tensor_digest(t)
    return {f"{prefix}.stat": np.array([d["sum"], d["l2"], d["absmax"]]), f"{prefix}.samples": d["samples"]}


def unet_case(H, W, S=2, seed=29):
    net = UNet(**ATTN0)
    deterministic_fill_(net.state_dict())
    net.double()                       # fp64: the near-zero bias gradients are then free of the reference's round-off
    x, angle, level, gy = (t.double() for t in inputs(seed, S, H, W))
    x.requires_grad_(True)
    y = net(x, angle, level)
    (y * gy).sum().backward()
    out = dict(seed=np.int64(seed), S=np.int64(S), H=np.int64(H), W=np.int64(W))
    out.update(digest("y", y))
    out.update(digest("gx", x.grad))
    out.update(grads_digest(net))
    np.savez_compressed(os.path.join(HERE, f"envelope_attn_{H}x{W}.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    unet_case(72, 72)
