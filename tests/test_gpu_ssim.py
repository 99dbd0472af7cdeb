"""ops.ssim / drivers.evaluate(ssim=True) on the GPU against the two CPU restatements of tests/ssim_ref.py.

The tolerance is not a constant: each case computes e = max |ssim_fp32 - ssim_fp64| on its own inputs (CPU, at test
time) and requires max |gpu - ssim_fp64| <= max(4 e, 1e-6) -- ssim_ref.bound.  The fp32 formula's own error is large on
flat images (the fp32 window does not sum to exactly 1, so E[x^2] - mu_x^2 does not cancel against C2 = 9e-4) and
depends on the summation order, so the kernel cannot be asked to match ssim_fp32 bit for bit there."""
import numpy as np
import pytest
import torch

import ssim_ref
from conftest import TINY

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _check(got, X, Y, tag, data_range=1.0):
    r64, e, bound = ssim_ref.bound(X, Y, data_range)
    err = float(np.abs(got.double().cpu().numpy() - r64).max())
    print(f"{tag}: ssim {r64[0]:+.6f}  e {e:.3e}  bound {bound:.3e}  |gpu - fp64| {err:.3e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == (X.shape[0],)
    assert err <= bound, (tag, err, bound)


@pytest.mark.parametrize("kind", ssim_ref.CLASSES)
@pytest.mark.parametrize("H,W", ssim_ref.SIZES + [(43, 75)])
def test_parity(dev, H, W, kind):
    """(43, 75): the valid map 33 x 65 is one pixel past a 32-tile boundary on both axes."""
    from view_fusion_amd import ops
    X, Y = ssim_ref.make_pair(kind, 2, 3, H, W)
    _check(ops.ssim(X.to(dev), Y.to(dev)), X, Y, f"{H}x{W} {kind}")


@pytest.mark.parametrize("kind", ssim_ref.CLASSES)
@pytest.mark.parametrize("B,C", [(1, 1), (1, 6), (16, 1), (16, 6), (16, 3)])
def test_parity_channels_and_batch(dev, B, C, kind):
    from view_fusion_amd import ops
    X, Y = ssim_ref.make_pair(kind, B, C, 43, 75, seed=1)
    _check(ops.ssim(X.to(dev), Y.to(dev)), X, Y, f"B={B} C={C} 43x75 {kind}")


def test_non_contiguous_input_equals_its_contiguous_copy(dev):
    from view_fusion_amd import ops
    X, Y = ssim_ref.make_pair("noisy", 3, 6, 48, 64)
    X, Y = X.to(dev), Y.to(dev)
    xv, yv = X[:, 1:4], Y[:, 1:4]                         # channel-sliced views
    assert not xv.is_contiguous()
    a, b = ops.ssim(xv, yv), ops.ssim(xv.contiguous(), yv.contiguous())
    assert torch.equal(a, b)
    _check(a, xv.cpu().contiguous(), yv.cpu().contiguous(), "channel slice")


def test_empty_batch(dev):
    from view_fusion_amd import ops
    out = ops.ssim(torch.empty(0, 3, 64, 64, device=dev), torch.empty(0, 3, 64, 64, device=dev))
    assert out.shape == (0,) and out.dtype == torch.float32 and out.device.type == "cuda"


def test_refuses_short_sides_and_cpu_tensors(dev):
    from view_fusion_amd import _lib, ops
    with pytest.raises(ValueError):
        ops.ssim(torch.rand(2, 3, 10, 64, device=dev), torch.rand(2, 3, 10, 64, device=dev))
    with pytest.raises(_lib.VFHipError):                  # no CPU fallback
        ops.ssim(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16))
    lib = _lib.load()                                      # the C ABI refuses the same geometry on its own
    assert lib.vf_ssim_workspace_floats(2, 3, 64, 64) == 2 * 3 * 4
    assert lib.vf_ssim(None, None, None, None, 2, 3, 10, 64, None, 1.0, None) != 0
    assert lib.vf_ssim(None, None, None, None, 2, 0, 64, 64, None, 1.0, None) != 0
    assert lib.vf_ssim(None, None, None, None, 0, 3, 64, 64, None, 1.0, None) == 0


def test_two_calls_are_bit_equal(dev):
    from view_fusion_amd import ops
    X, Y = ssim_ref.make_pair("noisy", 16, 3, 128, 128)
    X, Y = X.to(dev), Y.to(dev)
    assert torch.equal(ops.ssim(X, Y), ops.ssim(X, Y))


def test_graph_replay_is_bitwise(dev):
    from view_fusion_amd import ops
    pairs = [ssim_ref.make_pair(k, 4, 3, 43, 75, seed=s) for k, s in (("noisy", 2), ("rand_rand", 3))]
    eager = [ops.ssim(X.to(dev), Y.to(dev)) for X, Y in pairs]
    sx, sy = torch.zeros(4, 3, 43, 75, device=dev), torch.zeros(4, 3, 43, 75, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                            # one eager warm-up on the capture stream
        ops.ssim(sx, sy)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = ops.ssim(sx, sy)
    for (X, Y), want in zip(pairs, eager):
        sx.copy_(X)
        sy.copy_(Y)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


@pytest.mark.parametrize("kind", ssim_ref.CLASSES)
def test_data_range_255(dev, kind):
    from view_fusion_amd import ops
    X, Y = ssim_ref.make_pair(kind, 2, 3, 48, 64)
    X, Y = X * 255, Y * 255
    _check(ops.ssim(X.to(dev), Y.to(dev), data_range=255.0), X, Y, f"data_range=255 {kind}", data_range=255.0)


def _eval_setup(dev):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": dict(schedule="linear", num_timesteps=10, linear_start=1e-4, linear_end=0.09)})
    vf.set_new_noise_schedule(device=dev, phase="train")
    g = torch.Generator().manual_seed(700)
    hw = TINY["image_size"]
    batch = dict(target=torch.rand(3, 3, hw, hw, generator=g).to(dev), cond=torch.rand(3, 6, 3, hw, hw, generator=g).to(dev),
                 angle=torch.rand(3, 1, generator=g).to(dev), view_count=torch.tensor([2, 6, 3]))
    inject = dict(y_t=torch.randn(3, 3, hw, hw, generator=g).to(dev), z_seq=torch.randn(10, 3, 3, hw, hw, generator=g).to(dev))
    return vf, batch, inject


def test_evaluate_reports_ssim_and_leaves_psnr_alone(dev):
    from view_fusion_amd import drivers
    vf, batch, inject = _eval_setup(dev)
    both = drivers.evaluate(vf, [batch], ssim=True, **inject)
    alone = drivers.evaluate(vf, [batch], **inject)
    assert set(both) == {"psnr", "ssim"} and set(alone) == {"psnr"}
    assert torch.equal(both["psnr"], alone["psnr"])
    with torch.no_grad(), drivers._eval_mode(vf):
        *_, samples = vf(y_cond=batch["cond"], view_count=batch["view_count"], angle=batch["angle"], generate=True,
                         **inject)
    X, Y = samples.cpu(), batch["target"].cpu()
    r64, e, bound = ssim_ref.bound(X, Y)
    err = abs(float(both["ssim"]) - float(r64.mean()))
    print(f"evaluate: ssim {r64.mean():+.6f}  e {e:.3e}  bound {bound:.3e}  |gpu - fp64| {err:.3e}")
    assert both["ssim"].dim() == 0 and err <= bound
