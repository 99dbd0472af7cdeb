"""Pin the CPU oracle off the square power-of-two maps: it reproduces the reference's vectors at 24x40 and 20x20
(tests/golden/make_golden_envelope.py).  CPU only."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import unet_ref, view_fusion_ref as vfr
from view_fusion_amd.unet import UNet
from view_fusion_amd.utils import deterministic_fill_, tensor_digest

TINY3 = dict(in_channel=6, out_channel=6, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 2), attn_res=(4,),
             res_blocks=1, image_size=16)
SCHED_TRAIN = dict(schedule="linear", num_timesteps=2000, linear_start=1e-6, linear_end=1e-2)


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def filled_sd(hp):
    sd = UNet(**hp).state_dict()
    deterministic_fill_(sd)
    return {k: v.clone().requires_grad_(True) for k, v in sd.items()}


def check_grads(g, sd):
    for k, p in sd.items():
        ref = g[f"g.{k}.stat"]
        d = tensor_digest(p.grad)
        assert abs(d["l2"] - ref[1]) <= 1e-4 * ref[1] + 3e-5 * p.numel() ** 0.5, k
        if ref[2] < 1e-3:        # analytically ~0 (a bias in front of a GroupNorm): round-off only, the l2 bound covers it
            continue
        np.testing.assert_allclose(d["samples"], g[f"g.{k}.samples"], rtol=2e-3, atol=2e-5 * ref[2] + 3e-5, err_msg=k)


@pytest.mark.parametrize("hw", ["24x40", "20x20"])
def test_oracle_unet_off_square(hw):
    g = load(f"envelope_tiny3_{hw}.npz")
    sd = filled_sd(TINY3)
    x = torch.tensor(g["x"], requires_grad=True)
    y = unet_ref.unet_forward(sd, TINY3, x, torch.tensor(g["angle"]), torch.tensor(g["level"]))
    np.testing.assert_allclose(y.detach().numpy(), g["y"], rtol=1e-4, atol=5e-5)
    (y * torch.tensor(g["gy"])).sum().backward()
    np.testing.assert_allclose(x.grad.numpy(), g["gx"], rtol=1e-3, atol=1e-5)
    check_grads(g, sd)


def test_oracle_ragged_train_loss_off_square():
    g = load("envelope_train_ragged_24x40.npz")
    sd = filled_sd(TINY3)
    sched = vfr.schedule_buffers(vfr.beta_schedule(**SCHED_TRAIN))
    fn = lambda x, a, l: unet_ref.unet_forward(sd, TINY3, x, a, l)
    loss = vfr.train_loss(fn, sched, torch.tensor(g["y_cond"]), g["view_count"], torch.tensor(g["angle"]),
                          torch.tensor(g["y_0"]), torch.tensor(g["t"]), torch.tensor(g["u"]), torch.tensor(g["noise"]),
                          weighting=True)
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    loss.backward()
    check_grads(g, sd)
