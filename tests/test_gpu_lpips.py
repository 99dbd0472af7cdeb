"""ops.lpips / drivers.LPIPS / drivers.evaluate(lpips=) on the GPU against the two CPU restatements of
tests/lpips_ref.py.

The tolerance is not tuned to the kernels: each case computes r64 = lpips_fp64 and e = max |lpips_fp32 - r64| on its
own inputs and requires |gpu - r64| <= max(4 e, 1e-4 |r64| + 1e-6) per image (lpips_ref.bound).  Cases are computed
once (lpips_ref.case) and shared."""
import numpy as np
import pytest
import torch

import lpips_ref
from conftest import TINY

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_NETS = {}


def _net(dev, tap=None, dead_tail=False):
    from view_fusion_amd import drivers
    key = (tap, dead_tail)
    if key not in _NETS:
        ref = lpips_ref.net_cached(0, dead_tail)
        if tap is not None:
            ref = lpips_ref.only_tap(ref, tap)
        _NETS[key] = drivers.LPIPS.from_state_dicts(*ref).to(dev)
    return _NETS[key]


def _check(got, r64, e, bound, tag):
    err = np.abs(got.double().cpu().numpy() - r64)
    print(f"{tag}: lpips {r64[0]:.6e}  e {e:.3e}  bound {bound.max():.3e}  |gpu - fp64| {err.max():.3e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == r64.shape
    assert (err <= bound).all(), (tag, err, bound)


@pytest.mark.parametrize("kind,B,H,W", [(k, 2, 32, 32) for k in lpips_ref.KINDS] +
                         [("noisy", 2, 32, 64), ("noisy", 3, 64, 64), ("noisy", 1, 48, 80)])
def test_parity(dev, kind, B, H, W):
    """32x32: maps 32 ... 2, the deepest one float4.  32x64: non-square, deepest 2x4.  B=3 at 64x64: an odd batch on
    the specialised conv routes.  48x80: the last tap map is 3x5, H W % 4 != 0: the scalar tails run (ops.conv2d
    accepts every one of its maps through the any-size kernels, so the value is checked, not a refusal)."""
    from view_fusion_amd import ops
    X, Y, _, r64, e, bound = lpips_ref.case(kind, B, H, W)
    got = ops.lpips(X.to(dev), Y.to(dev), _net(dev))
    _check(got, r64, e, bound, f"B={B} {H}x{W} {kind}")
    if kind == "identical":
        assert float(got.abs().max()) <= 1e-8


@pytest.mark.parametrize("tap", range(5))
def test_each_tap_alone(dev, tap):
    """All lin weights zero except one tap's: a tap taken after the pool, or a dropped layer, shows here."""
    from view_fusion_amd import ops
    X, Y, _, r64, e, bound = lpips_ref.case("unrelated", 2, 32, 32, tap=tap)
    assert (r64 > 50 * bound).all()                        # the tap's term stands well clear of the tolerance
    _check(ops.lpips(X.to(dev), Y.to(dev), _net(dev, tap=tap)), r64, e, bound, f"tap {tap} alone")


def test_dead_tap_sits_on_the_epsilon(dev):
    """relu5_3 all zero for both images: 0 / (0 + 1e-10) per channel, no NaN, the tap adds exactly nothing."""
    from view_fusion_amd import drivers
    X, Y, _, r64, e, bound = lpips_ref.case("noisy", 2, 32, 32, dead_tail=True)
    got = drivers.compute_lpips(X.to(dev), Y.to(dev), _net(dev, dead_tail=True))
    assert torch.isfinite(got).all()
    _check(got, r64, e, bound, "dead tail")


def test_value_does_not_depend_on_the_batch(dev):
    X, Y, _, r64, e, bound = lpips_ref.case("noisy", 3, 64, 64)
    net = _net(dev)
    Xd, Yd = X.to(dev), Y.to(dev)
    for b in range(3):
        _check(net(Xd[b:b + 1], Yd[b:b + 1]), r64[b:b + 1], e, bound[b:b + 1], f"pair {b} of 3, alone")


def test_non_contiguous_input_equals_its_contiguous_copy(dev):
    from view_fusion_amd import ops
    g = torch.Generator().manual_seed(5)
    X, Y = torch.rand(2, 6, 32, 32, generator=g).to(dev), torch.rand(2, 6, 32, 32, generator=g).to(dev)
    xv, yv = X[:, 1:4], Y[:, 2:5]                         # channel-sliced views
    assert not xv.is_contiguous()
    a, b = ops.lpips(xv, yv, _net(dev)), ops.lpips(xv.contiguous(), yv.contiguous(), _net(dev))
    assert torch.equal(a, b) and float(a.min()) > 0


def test_empty_batch_and_bad_sizes(dev):
    from view_fusion_amd import _lib, ops
    net = _net(dev)
    out = ops.lpips(torch.empty(0, 3, 32, 32, device=dev), torch.empty(0, 3, 32, 32, device=dev), net)
    assert out.shape == (0,) and out.dtype == torch.float32 and out.device.type == "cuda"
    for shape in [(2, 3, 16, 32), (2, 3, 32, 40), (2, 3, 72, 64), (2, 4, 32, 32)]:
        with pytest.raises(ValueError):
            ops.lpips(torch.rand(*shape, device=dev), torch.rand(*shape, device=dev), net)
    with pytest.raises(ValueError):
        ops.lpips(torch.rand(2, 3, 32, 32, device=dev), torch.rand(2, 3, 32, 64, device=dev), net)
    lib = _lib.load()                                      # the C ABI refuses bad geometry on its own
    assert lib.vf_lpips_workspace_floats(2, 32, 40) == 0 and lib.vf_lpips_workspace_floats(2, 32, 32) > 0
    assert lib.vf_relu_maxpool2(None, None, 4, 3, 4, None) != 0
    assert lib.vf_lpips_layer(None, None, None, 2, 64, 16, 0, 0, None) != 0          # no room for its slot
    assert lib.vf_lpips_layer(None, None, None, 0, 64, 16, 0, 1, None) == 0


def test_graph_replay_and_two_eager_calls_are_bitwise(dev):
    from view_fusion_amd import ops
    net = _net(dev)
    pairs = [lpips_ref.case(k, 2, 32, 32)[:2] for k in ("noisy", "unrelated")]
    eager = [ops.lpips(X.to(dev), Y.to(dev), net) for X, Y in pairs]
    again = [ops.lpips(X.to(dev), Y.to(dev), net) for X, Y in pairs]
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    sx, sy = torch.zeros(2, 3, 32, 32, device=dev), torch.zeros(2, 3, 32, 32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                            # one eager warm-up on the capture stream: packs, workspace
        ops.lpips(sx, sy, net)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = ops.lpips(sx, sy, net)
    for (X, Y), want in zip(pairs, eager):
        sx.copy_(X)
        sy.copy_(Y)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def test_evaluate_reports_lpips_next_to_psnr_and_ssim(dev):
    """A 9-step schedule: generate() keeps 8 intermediate samples and asserts num_timesteps > 8, so 9 is the shortest
    chain evaluate() can drive."""
    from view_fusion_amd import UNet, ViewFusion, drivers, ops
    from view_fusion_amd.utils import deterministic_fill_
    hp = dict(TINY, image_size=32)
    unet = UNet(**hp)
    deterministic_fill_(unet.state_dict())
    vf = ViewFusion(unet.to(dev), {"train": dict(schedule="linear", num_timesteps=9, linear_start=1e-4, linear_end=0.09)})
    vf.set_new_noise_schedule(device=dev, phase="train")
    g = torch.Generator().manual_seed(701)
    batch = dict(target=torch.rand(2, 3, 32, 32, generator=g).to(dev), cond=torch.rand(2, 6, 3, 32, 32, generator=g).to(dev),
                 angle=torch.rand(2, 1, generator=g).to(dev), view_count=torch.tensor([2, 5]))
    net = _net(dev)
    out = drivers.evaluate(vf, [batch], ssim=True, lpips=net, seed=0)
    assert set(out) == {"psnr", "ssim", "lpips"}
    assert set(drivers.evaluate(vf, [batch], ssim=True, seed=0)) == {"psnr", "ssim"}
    with torch.no_grad(), drivers._eval_mode(vf):
        *_, samples = vf(y_cond=batch["cond"], view_count=batch["view_count"], angle=batch["angle"], generate=True,
                         seed=0, sample_ids=torch.arange(2))
    want = ops.lpips(samples, batch["target"], net).mean()
    assert out["lpips"].dim() == 0 and torch.equal(out["lpips"], want) and float(want) > 0
