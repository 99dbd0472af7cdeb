"""The UNet / ViewFusion with attention maps above 4096 pixels (the streaming attention kernels) on a real MI355X against
the CPU oracle and a reference-made fixture: training, replayed training and the sampler, at the tolerances of
tests/test_gpu_envelope_model.py."""
import copy
import math

import numpy as np
import pytest
import torch

from test_gpu_envelope_model import _check_digests, _load, make_unet

pytestmark = pytest.mark.gpu
SCHED_TRAIN = dict(schedule="linear", num_timesteps=2000, linear_start=1e-6, linear_end=1e-2)
# attention on level 0 (72x72: L = 5184, streaming); the mid block adds attention on level 1 (36x36: L = 1296, generic)
ATTN0 = dict(in_channel=6, out_channel=6, inner_channel=32, norm_groups=32, channel_mults=(1, 2), attn_res=(16,),
             res_blocks=1, image_size=16)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _sd64(net):
    return {k: v.detach().cpu().double().requires_grad_(True) for k, v in net.state_dict().items()}


def _unet_vs_oracle64(dev, hp, S, H, W, seed):
    """The checks and tolerances of test_gpu_envelope_model._unet_vs_oracle, with the oracle run in fp64: at 5184+
    pixels the fp32 oracle's own round-off on the near-zero bias gradients in front of a GroupNorm is as large as the
    bound."""
    from oracle import unet_ref
    net = make_unet(hp, dev)
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(S, hp["in_channel"], H, W, generator=g)
    angle = 2 * np.pi / 24 * torch.randint(0, 24, (S, 1), generator=g).float()
    level = torch.rand(S, 1, generator=g)
    xg = x.to(dev).requires_grad_(True)
    y = net(xg, angle.to(dev), level.to(dev))
    gy = torch.randn(y.shape, generator=g)
    (y * gy.to(dev)).sum().backward()
    sd = _sd64(net)
    xc = x.double().requires_grad_(True)
    yc = unet_ref.unet_forward(sd, hp, xc, angle.double(), level.double())
    (yc * gy.double()).sum().backward()
    np.testing.assert_allclose(y.detach().cpu().numpy(), yc.detach().numpy(), rtol=1e-4, atol=5e-5)
    assert float((xg.grad.cpu().double() - xc.grad).norm() / xc.grad.norm()) < 1e-4
    for k, p in net.named_parameters():
        a, b = p.grad.detach().cpu().double(), sd[k].grad
        assert float((a - b).norm()) <= 1e-4 * float(b.norm()) + 3e-5 * b.numel() ** 0.5, k
    with torch.no_grad():                      # the no-grad (sampler) forward
        yi = net(x.to(dev), angle.to(dev), level.to(dev))
    np.testing.assert_allclose(yi.cpu().numpy(), yc.detach().numpy(), rtol=1e-4, atol=5e-5)


@pytest.mark.parametrize("S,H,W", [(2, 72, 72), (2, 64, 80), (1, 128, 128)], ids=lambda v: str(v))
def test_attn0_forward_backward_vs_oracle(dev, S, H, W):
    """72x72 and 64x80: level 0 streams (L = 5184 / 5120), the mid block stays generic; 128x128: level 0 L = 16384
    streams, the mid block's L = 4096 stays generic."""
    _unet_vs_oracle64(dev, ATTN0, S, H, W, 11)


def test_attn0_vs_reference_vectors_72x72(dev):
    """tests/golden/envelope_attn_72x72.npz, made by the reference itself (inputs re-drawn from the stored seed)."""
    g = _load("envelope_attn_72x72.npz")
    S, H, W = int(g["S"]), int(g["H"]), int(g["W"])
    gen = torch.Generator().manual_seed(int(g["seed"]))
    x = torch.rand(S, 6, H, W, generator=gen)
    angle = 2 * np.pi / 24 * torch.randint(0, 24, (S, 1), generator=gen).float()
    level = torch.rand(S, 1, generator=gen)
    gy = torch.randn(S, 6, H, W, generator=gen)
    from view_fusion_amd.utils import tensor_digest
    net = make_unet(ATTN0, dev)
    xg = x.to(dev).requires_grad_(True)
    y = net(xg, angle.to(dev), level.to(dev))
    (y * gy.to(dev)).sum().backward()
    for name, t in (("y", y), ("gx", xg.grad)):
        d, ref = tensor_digest(t), g[f"{name}.stat"]
        assert abs(d["l2"] - ref[1]) <= 1e-4 * ref[1], name
        np.testing.assert_allclose(d["samples"], g[f"{name}.samples"], rtol=1e-3, atol=5e-5, err_msg=name)
    _check_digests(g, net.named_parameters())


def test_attn0_ragged_train_72x72_vs_oracle(dev):
    from oracle import unet_ref, view_fusion_ref as vfr
    from view_fusion_amd import ViewFusion
    vf = ViewFusion(make_unet(ATTN0, dev), {"train": SCHED_TRAIN}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    B, N, H, W = 2, 3, 72, 72
    g = torch.Generator().manual_seed(12)
    y_0, y_cond = torch.rand(B, 3, H, W, generator=g), torch.rand(B, N, 3, H, W, generator=g)
    angle = 2 * np.pi / 24 * torch.randint(0, 24, (B, 1), generator=g).float()
    noise, t, u = torch.randn(B, 3, H, W, generator=g), torch.tensor([1500, 3]), torch.rand(B, 1, generator=g)
    vc = torch.tensor([3, 1])
    loss = vf(y_cond=y_cond.to(dev), view_count=vc, angle=angle.to(dev), y_0=y_0.to(dev), noise=noise.to(dev),
              t=t.to(dev), u=u.to(dev))
    loss.backward()
    sd = _sd64(vf.denoise_fn)                  # fp64 oracle, as _unet_vs_oracle64
    sched = vfr.schedule_buffers(vfr.beta_schedule(**SCHED_TRAIN))
    d = lambda z: z.double()  # noqa: E731
    lref = vfr.train_loss(lambda x, a, l: unet_ref.unet_forward(sd, ATTN0, x, a, l), sched, d(y_cond), vc, d(angle),
                          d(y_0), t, d(u), d(noise), True)
    lref.backward()
    assert abs(loss.item() - lref.item()) <= 1e-5 * abs(lref.item())
    worst = 0.0
    for k, p in vf.denoise_fn.named_parameters():
        a, b = p.grad.detach().cpu().double(), sd[k].grad.double()
        if float(b.norm()) > 1e-4:
            worst = max(worst, float((a - b).norm() / b.norm()))
    assert worst < 1e-4, worst


def test_attn0_trainer_graph_replay_72x72_matches_eager_bitwise(dev):
    from view_fusion_amd import train
    ma = train.build_model(unet_params=ATTN0, device="cuda:0", seed=3)
    mb = copy.deepcopy(ma)
    ta, tb = train.Trainer(ma, graph=False, lr_warmup=4), train.Trainer(mb, graph=True, lr_warmup=4)
    B, N, H, W, n = 2, 2, 72, 72, 5
    for i in range(n):
        g = torch.Generator().manual_seed(200 + i)
        bt = dict(y_0=torch.rand(B, 3, H, W, generator=g).to(dev), y_cond=torch.rand(B, N, 3, H, W, generator=g).to(dev),
                  angle=(2 * math.pi / 24 * torch.randint(0, 24, (B, 1), generator=g).float()).to(dev),
                  view_count=torch.full((B,), N))
        dr = dict(t=torch.randint(1, 2000, (B,), generator=g).to(dev), u=torch.rand(B, 1, generator=g).to(dev),
                  noise=torch.randn(B, 3, H, W, generator=g).to(dev))
        la, lb = ta.step(bt, **dr), tb.step(bt, **dr)
        assert torch.equal(la, lb), i
        for (k, p), q in zip(ma.named_parameters(), mb.parameters()):
            assert torch.equal(p, q), (i, k)
    assert tb.graph_steps == n - train.Trainer.GRAPH_AFTER > 0
    for p, q in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(p.grad, q.grad)


@pytest.mark.parametrize("N", [1, 6])
def test_attn0_generate_chain_72x72_vs_oracle(dev, N):
    """generate() at B = 1: the captured reverse step (streaming attention inside the graph) equals the eager chain bit
    for bit, and both match the oracle."""
    from oracle import unet_ref, view_fusion_ref as vfr
    from view_fusion_amd import ViewFusion
    steps = 10                                 # generate() keeps sample_num = 8 intermediate images: T > 8
    sched_kw = dict(schedule="linear", num_timesteps=steps, linear_start=1e-4, linear_end=0.09)
    vf = ViewFusion(make_unet(ATTN0, dev), {"train": sched_kw}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    H, W = 72, 72
    g = torch.Generator().manual_seed(400 + N)
    y_cond = torch.rand(1, N, 3, H, W, generator=g)
    angle = 2 * np.pi / 24 * torch.randint(0, 24, (1, 1), generator=g).float()
    y_T = torch.randn(1, 3, H, W, generator=g)
    z_seq = torch.randn(steps, 1, 3, H, W, generator=g)
    vc = torch.tensor([N])
    outs = {}
    for use_graph in (True, False):
        outs[use_graph] = [t.cpu() for t in vf.generate(y_cond.to(dev), vc, angle.to(dev), y_t=y_T.to(dev),
                                                        z_seq=z_seq.to(dev), use_graph=use_graph)[:4]]
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)
    y, ret, logit_arr, weight_arr = outs[True]
    sd = {k: v.detach().cpu() for k, v in vf.denoise_fn.state_dict().items()}
    sched = vfr.schedule_buffers(vfr.beta_schedule(**sched_kw))
    with torch.no_grad():
        yr, retr, lr, wr, _ = vfr.generate(lambda x, a, l: unet_ref.unet_forward(sd, ATTN0, x, a, l), sched, y_cond, vc,
                                           angle, y_T, z_seq)
    np.testing.assert_allclose(y.numpy(), yr.numpy(), rtol=1e-4, atol=5e-5)
    np.testing.assert_allclose(ret.numpy(), retr.numpy(), rtol=1e-4, atol=5e-5)
    np.testing.assert_allclose(logit_arr.numpy(), lr.numpy(), rtol=1e-4, atol=5e-5)
    np.testing.assert_allclose(weight_arr.numpy(), wr.numpy(), rtol=1e-4, atol=1e-5)
