"""The UNet / ViewFusion at input sizes outside the square power-of-two envelope of the specialised kernels (non-square,
non-power-of-two, a 4x4 bottom map) on a real MI355X against the CPU oracle, at the tolerances of tests/test_gpu_model.py;
and the ValueError for a size the reference itself cannot run."""
import numpy as np
import pytest
import torch

from conftest import SMALL

pytestmark = pytest.mark.gpu
SCHED_TRAIN = dict(schedule="linear", num_timesteps=2000, linear_start=1e-6, linear_end=1e-2)
SCHED_TEST = dict(schedule="linear", num_timesteps=1000, linear_start=1e-4, linear_end=0.09)
# TINY with a third level (two Downsamples); attention on the bottom map (6x10 at 24x40, 5x5 at 20x20)
TINY3 = dict(in_channel=6, out_channel=6, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 2), attn_res=(4,),
             res_blocks=1, image_size=16)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_unet(hp, dev):
    from view_fusion_amd import UNet
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**hp)
    deterministic_fill_(net.state_dict())
    return net.to(dev)


def cpu_sd(net):
    return {k: v.detach().cpu().clone().requires_grad_(True) for k, v in net.state_dict().items()}


def _unet_vs_oracle(dev, hp, S, H, W, seed):
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
    sd = cpu_sd(net)
    xc = x.clone().requires_grad_(True)
    yc = unet_ref.unet_forward(sd, hp, xc, angle, level)
    (yc * gy).sum().backward()
    np.testing.assert_allclose(y.detach().cpu().numpy(), yc.detach().numpy(), rtol=1e-4, atol=5e-5)
    assert float((xg.grad.cpu() - xc.grad).norm() / xc.grad.norm()) < 1e-4
    for k, p in net.named_parameters():
        a, b = p.grad.detach().cpu().double(), sd[k].grad.double()
        assert float((a - b).norm()) <= 1e-4 * float(b.norm()) + 3e-5 * b.numel() ** 0.5, k
    with torch.no_grad():                      # the no-grad (sampler) forward: split-K / fused-GroupNorm routes
        yi = net(x.to(dev), angle.to(dev), level.to(dev))
    np.testing.assert_allclose(yi.cpu().numpy(), yc.detach().numpy(), rtol=1e-4, atol=5e-5)


@pytest.mark.parametrize("hw", [(24, 40), (20, 20)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny3_forward_backward_vs_oracle(dev, hw):
    _unet_vs_oracle(dev, TINY3, 3, hw[0], hw[1], 1)


@pytest.mark.parametrize("hw", [(48, 64), (32, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_forward_backward_vs_oracle(dev, hw):
    """The SMALL config (33.9 M parameters): 48x64 (12x16 attention, 6x8 bottom) and 32x32 (4x4 bottom map)."""
    _unet_vs_oracle(dev, SMALL, 2, hw[0], hw[1], 2)


def test_small_ragged_train_step_48x64_vs_oracle(dev):
    from oracle import unet_ref, view_fusion_ref as vfr
    from view_fusion_amd import ViewFusion
    vf = ViewFusion(make_unet(SMALL, dev), {"train": SCHED_TRAIN}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    B, N, H, W = 2, 3, 48, 64
    g = torch.Generator().manual_seed(4)
    y_0, y_cond = torch.rand(B, 3, H, W, generator=g), torch.rand(B, N, 3, H, W, generator=g)
    angle = 2 * np.pi / 24 * torch.randint(0, 24, (B, 1), generator=g).float()
    noise, t, u = torch.randn(B, 3, H, W, generator=g), torch.tensor([1500, 3]), torch.rand(B, 1, generator=g)
    vc = torch.tensor([3, 1])
    loss = vf(y_cond=y_cond.to(dev), view_count=vc, angle=angle.to(dev), y_0=y_0.to(dev), noise=noise.to(dev),
              t=t.to(dev), u=u.to(dev))
    loss.backward()
    sd = cpu_sd(vf.denoise_fn)
    sched = vfr.schedule_buffers(vfr.beta_schedule(**SCHED_TRAIN))
    lref = vfr.train_loss(lambda x, a, l: unet_ref.unet_forward(sd, SMALL, x, a, l), sched, y_cond, vc, angle, y_0, t, u,
                          noise, True)
    lref.backward()
    assert abs(loss.item() - lref.item()) <= 1e-5 * abs(lref.item())
    worst = 0.0
    for k, p in vf.denoise_fn.named_parameters():
        a, b = p.grad.detach().cpu().double(), sd[k].grad.double()
        if float(b.norm()) > 1e-4:
            worst = max(worst, float((a - b).norm() / b.norm()))
    assert worst < 1e-4, worst


@pytest.mark.parametrize("N", [1, 6])
def test_small_reverse_step_48x64_vs_oracle(dev, N):
    """One sampler step (p_sample, no autograd) at B = 1: the split-K direct convs of the general kernel."""
    from oracle import unet_ref, view_fusion_ref as vfr
    from view_fusion_amd import ViewFusion
    vf = ViewFusion(make_unet(SMALL, dev), {"train": SCHED_TEST}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    B, H, W = 1, 48, 64
    g = torch.Generator().manual_seed(6)
    y_t, y_cond = torch.rand(B, 3, H, W, generator=g), torch.rand(B, N, 3, H, W, generator=g)
    angle = 2 * np.pi / 24 * torch.randint(0, 24, (B, 1), generator=g).float()
    vc, t, z = torch.tensor([N]), torch.tensor([500]), torch.randn(B, 3, H, W, generator=g)
    with torch.no_grad():
        y, _, w = vf.p_sample(y_t.to(dev), y_cond.to(dev), vc, angle.to(dev), t.to(dev), z=z.to(dev))
        sd = {k: v.detach().cpu() for k, v in vf.denoise_fn.state_dict().items()}
        buf = vfr.schedule_buffers(vfr.beta_schedule(**SCHED_TEST))
        yr, _, wr = vfr.p_sample(lambda x, a, l: unet_ref.unet_forward(sd, SMALL, x, a, l), buf, y_t, y_cond, vc, angle,
                                 t, z)
    assert float((y.cpu() - yr).abs().max()) < 5e-5 and float((w.cpu() - wr).abs().max()) < 1e-5


def _load(name):
    import os
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, name))


def _check_digests(g, named_params):
    from view_fusion_amd.utils import tensor_digest
    for k, p in named_params:
        ref = g[f"g.{k}.stat"]
        d = tensor_digest(p.grad)
        assert abs(d["l2"] - ref[1]) <= 1e-4 * ref[1] + 3e-5 * p.numel() ** 0.5, k
        if ref[2] < 1e-3:        # analytically ~0 (a bias in front of a GroupNorm): round-off only, the l2 bound covers it
            continue
        np.testing.assert_allclose(d["samples"], g[f"g.{k}.samples"], rtol=2e-3, atol=2e-5 * ref[2] + 3e-5, err_msg=k)


@pytest.mark.parametrize("hw", ["24x40", "20x20"])
def test_tiny3_vs_reference_vectors(dev, hw):
    """tests/golden/envelope_tiny3_*.npz, made by the reference itself."""
    g = _load(f"envelope_tiny3_{hw}.npz")
    net = make_unet(TINY3, dev)
    x = torch.tensor(g["x"]).to(dev).requires_grad_(True)
    y = net(x, torch.tensor(g["angle"]).to(dev), torch.tensor(g["level"]).to(dev))
    np.testing.assert_allclose(y.detach().cpu().numpy(), g["y"], rtol=1e-4, atol=5e-5)
    (y * torch.tensor(g["gy"]).to(dev)).sum().backward()
    np.testing.assert_allclose(x.grad.cpu().numpy(), g["gx"], rtol=1e-3, atol=3e-5)
    _check_digests(g, net.named_parameters())


def test_ragged_train_24x40_vs_reference_vectors(dev):
    from view_fusion_amd import ViewFusion
    g = _load("envelope_train_ragged_24x40.npz")
    vf = ViewFusion(make_unet(TINY3, dev), {"train": SCHED_TRAIN}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    T = lambda k: torch.tensor(g[k]).to(dev)
    loss = vf(y_cond=T("y_cond"), view_count=torch.tensor(g["view_count"]), angle=T("angle"), y_0=T("y_0"),
              noise=T("noise"), t=T("t"), u=T("u"))
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    loss.backward()
    _check_digests(g, vf.denoise_fn.named_parameters())


def test_size_outside_the_reference_envelope_raises_value_error(dev):
    net = make_unet(TINY3, dev)
    x = torch.rand(2, 6, 18, 18, device=dev)
    a = torch.rand(2, 1, device=dev)
    with pytest.raises(ValueError, match="18x18"):
        net(x, a, a)


def test_trainer_graph_replay_48x64_matches_eager_bitwise(dev):
    """Trainer(graph=True) at 48x64 (the general kernels inside a captured iteration, pack plan for that size) against
    the same iterations enqueued eagerly: parameters, gradients and losses bit for bit."""
    import copy
    import math
    from view_fusion_amd import train
    ma = train.build_model(unet_params=SMALL, device="cuda:0", seed=3)
    mb = copy.deepcopy(ma)
    ta, tb = train.Trainer(ma, graph=False, lr_warmup=4), train.Trainer(mb, graph=True, lr_warmup=4)
    B, N, H, W, n = 4, 2, 48, 64, 5
    for i in range(n):
        g = torch.Generator().manual_seed(100 + i)
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
def test_small_generate_chain_48x64_vs_oracle(dev, N):
    """generate() at B = 1, 48x64: the reverse step captured into a HIP graph and replayed (the default at S <= 16), with
    the split-K general convs and the unfused conv + GroupNorm route, over 12 steps against the oracle; the captured and
    the eager chain are bitwise equal."""
    from oracle import unet_ref, view_fusion_ref as vfr
    from view_fusion_amd import ViewFusion
    sched_kw = dict(schedule="linear", num_timesteps=12, linear_start=1e-4, linear_end=0.09)
    vf = ViewFusion(make_unet(SMALL, dev), {"train": sched_kw}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    H, W = 48, 64
    g = torch.Generator().manual_seed(300 + N)
    y_cond = torch.rand(1, N, 3, H, W, generator=g)
    angle = 2 * np.pi / 24 * torch.randint(0, 24, (1, 1), generator=g).float()
    y_T = torch.randn(1, 3, H, W, generator=g)
    z_seq = torch.randn(12, 1, 3, H, W, generator=g)
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
        yr, retr, lr, wr, _ = vfr.generate(lambda x, a, l: unet_ref.unet_forward(sd, SMALL, x, a, l), sched, y_cond, vc,
                                           angle, y_T, z_seq)
    np.testing.assert_allclose(y.numpy(), yr.numpy(), rtol=1e-4, atol=5e-5)
    np.testing.assert_allclose(ret.numpy(), retr.numpy(), rtol=1e-4, atol=5e-5)
    np.testing.assert_allclose(logit_arr.numpy(), lr.numpy(), rtol=1e-4, atol=5e-5)
    np.testing.assert_allclose(weight_arr.numpy(), wr.numpy(), rtol=1e-4, atol=1e-5)
