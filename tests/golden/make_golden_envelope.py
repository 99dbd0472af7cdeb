#!/usr/bin/env python3
"""Golden vectors off the square power-of-two maps, from the REAL reference (see make_golden.py for how the reference
is reached; run in the build container only):

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_envelope.py

  envelope_tiny3_24x40.npz / envelope_tiny3_20x20.npz
        TINY with a third channel mult (two Downsamples): attention on a 6x10 map (L = 60) at 24x40, a 5x5 bottom map at
        20x20.  UNet forward output, input gradient and digests of every parameter gradient.
  envelope_train_ragged_24x40.npz
        ViewFusion train loss + gradient digests at 24x40, ragged view_count, weighting on.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import SCHEDULES, UNet, deterministic_fill_, grads_digest, make_vf  # noqa: E402

TINY3 = dict(in_channel=6, out_channel=6, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 2), attn_res=(4,),
             res_blocks=1, image_size=16)


def unet_case(H, W):
    net = UNet(**TINY3)
    deterministic_fill_(net.state_dict())
    g = torch.Generator().manual_seed(17)
    S = 3
    x = torch.rand(S, 6, H, W, generator=g)
    angle = 2 * np.pi / 24 * torch.randint(0, 24, (S, 1), generator=g).float()
    level = torch.rand(S, 1, generator=g)
    x.requires_grad_(True)
    y = net(x, angle, level)
    gy = torch.randn(y.shape, generator=g)
    (y * gy).sum().backward()
    out = dict(x=x.detach().numpy(), angle=angle.numpy(), level=level.numpy(), y=y.detach().numpy(), gy=gy.numpy(),
               gx=x.grad.numpy())
    out.update(grads_digest(net))
    np.savez_compressed(os.path.join(HERE, f"envelope_tiny3_{H}x{W}.npz"), **out)


def train_case(H, W):
    vf = make_vf(TINY3, SCHEDULES["linear_train"], True)
    B, N = 3, 3
    g = torch.Generator().manual_seed(19)
    y_0, y_cond = torch.rand(B, 3, H, W, generator=g), torch.rand(B, N, 3, H, W, generator=g)
    angle = 2 * np.pi / 24 * torch.randint(0, 24, (B, 1), generator=g).float()
    noise = torch.randn(B, 3, H, W, generator=g)
    vc = torch.tensor([1, 3, 2], dtype=torch.long)
    torch.manual_seed(123)          # the reference draws t, u from the global generator: record the same two draws
    t = torch.randint(1, vf.num_timesteps, (B,)).long()
    u = torch.rand((B, 1))
    torch.manual_seed(123)
    loss = vf(y_cond=y_cond, view_count=vc, angle=angle, y_0=y_0, noise=noise)
    loss.backward()
    out = dict(y_0=y_0.numpy(), y_cond=y_cond.numpy(), angle=angle.numpy(), noise=noise.numpy(), view_count=vc.numpy(),
               t=t.numpy(), u=u.numpy(), loss=np.float64(loss.item()))
    out.update(grads_digest(vf.denoise_fn))
    np.savez_compressed(os.path.join(HERE, f"envelope_train_ragged_{H}x{W}.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    unet_case(24, 40)
    unet_case(20, 20)
    train_case(24, 40)
