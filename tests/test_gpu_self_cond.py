"""Self-conditioning on the GPU (the head of csrc/diffusion.hip holds the definition): the three kernels against the
restatement of tests/selfcond_ref.py, the first pass and forward() against the two-pass chain through the oracle UNet
(with the check that a gradient flowing through the first pass would be noticed), the self-conditioned samplers against
the float64 chain, the Trainer (graph replay, injected draws, accum_steps) and the untouched default paths.

Tolerances, the project's own: one kernel rel 2e-5 (max|a-b| / max|b|); a chain through the UNet max-abs 1e-3; the loss
tests' close() (1e-6 relative + 1e-7); a parameter gradient ||g - ref|| <= 1e-4 ||ref|| + 3e-5 sqrt(numel) (test_gpu_model.py's
l2 bound with its per-element floor); "bitwise" is torch.equal."""
import numpy as np
import pytest
import torch

import guidance_ref
import prediction_ref
import sampler_ref
import selfcond_ref
from conftest import TINY

pytestmark = pytest.mark.gpu
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
T = SCHED["num_timesteps"]
# the loss tests' shapes: less than one workgroup of float4s; a count that is no multiple of 256; more than the 64-chunk
# grid covers in one pass (the grid-stride loop)
SHAPES = {"8x8": ((8, 8), (1, 3, 2)), "12x20": ((12, 20), (1, 3, 2)), "128x192": ((128, 192), (2,))}
KERNEL_RTOL, CHAIN_TOL = 2e-5, 1e-3
VC = [1, 3, 2]
IDS = [3, 2 ** 33 + 9, 14]
SEED = 32
WIDE = {3: dict(TINY, in_channel=9), 6: dict(TINY, in_channel=12)}
NEW = {"vf_stack_views_sc", "vf_draw_self_cond", "vf_self_cond_estimate"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def rel(a, b):
    a, b = (torch.as_tensor(x).detach().double().cpu().numpy() for x in (a, b))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def maxabs(a, b):
    a, b = (torch.as_tensor(x).detach().double().cpu().numpy() for x in (a, b))
    return float(np.abs(a - b).max())


def close(a, b):
    """test_gpu_loss_options.py's loss tolerance, element by element."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) < 1e-6 * np.abs(b) + 1e-7))


def grad_miss(got, ref):
    """How far a gradient is beyond the gradient tolerance: ||got - ref|| / (1e-4 ||ref|| + 3e-5 sqrt(numel)); <= 1 passes."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / (1e-4 * ref.norm() + 3e-5 * ref.numel() ** 0.5))


def _gammas32():
    from oracle import view_fusion_ref as vfr
    return vfr.schedule_buffers(vfr.beta_schedule(**SCHED))["gammas"].numpy()


def _betas():
    from view_fusion_amd import schedule
    return np.asarray(schedule.make_beta_schedule(**SCHED), dtype=np.float64)


# ---- 1. ops: stacking ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [3, 6])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_stack_views_self_cond(dev, shape, Cc):
    from view_fusion_amd import ops
    (H, W), vc = SHAPES[shape]
    B, S = len(vc), sum(vc)
    g = torch.Generator().manual_seed(3 + H + Cc)
    y_cond = torch.rand(B, max(vc), Cc, H, W, generator=g)
    y_t, noise, sc = (torch.randn(B, 3, H, W, generator=g) for _ in range(3))
    level, angle = torch.rand(B, generator=g) * 0.98 + 0.01, torch.rand(B, 1, generator=g)
    mask = torch.tensor([True, False, True][:B])
    off, _, _ = ops.view_offsets(list(vc), dev)
    off1, _, _ = ops.view_offsets([1] * B, dev)
    d = lambda t: None if t is None else t.to(dev)                                     # noqa: E731
    for nz in (noise, None):
        # the noisy target as the EXISTING kernel forms it (selfcond_ref.stack takes it as given)
        tgt = ops.stack_views(torch.zeros(B, 1, Cc, H, W, device=dev), d(y_t), d(nz), d(level), d(angle), off1, B)[0][:, Cc:]
        for drop in (None, mask):
            for null in (False, True):
                base = ops.stack_views(d(y_cond), d(y_t), d(nz), d(level), d(angle), off, S, drop=d(drop), null_rows=null)
                for est in (sc, None):
                    x, ls, as_ = ops.stack_views(d(y_cond), d(y_t), d(nz), d(level), d(angle), off, S, drop=d(drop),
                                                 null_rows=null, self_cond=d(est), sc_channels=True)
                    rows = S + B if null else S
                    assert x.shape == (rows, Cc + 6, H, W) and ls.shape == as_.shape == (rows, 1)
                    # the first Cc + 3 channels, the levels and the angles: the existing kernels' bits
                    assert torch.equal(x[:, :Cc + 3], base[0]) and torch.equal(ls, base[1]) and torch.equal(as_, base[2])
                    want, wa, wl = selfcond_ref.stack(y_cond, vc, tgt.cpu(), level.reshape(-1, 1), angle,
                                                      drop=None if drop is None else drop.numpy(), null_rows=null, sc=est)
                    assert torch.equal(x.cpu(), want) and torch.equal(ls.cpu(), wl) and torch.equal(as_.cpu(), wa)
    # a self_cond tensor alone selects the kernel as well
    x2 = ops.stack_views(d(y_cond), d(y_t), None, d(level), d(angle), off, S, self_cond=d(sc))[0]
    assert torch.equal(x2, ops.stack_views(d(y_cond), d(y_t), None, d(level), d(angle), off, S, self_cond=d(sc),
                                           sc_channels=True)[0])
    # copy_cond=False: the conditioning part of a pre-filled x is untouched, the other two parts are rewritten
    pre = torch.full((S + B, Cc + 6, H, W), float("nan"), device=dev)
    ops.stack_views(d(y_cond), d(y_t), None, d(level), d(angle), off, S, x=pre, copy_cond=False, null_rows=True, drop=d(mask),
                    self_cond=d(sc))
    rows = torch.cat([torch.repeat_interleave(torch.arange(B), torch.tensor(vc)), torch.arange(B)]).to(dev)
    assert torch.isnan(pre[:, :Cc]).all() and torch.equal(pre[:, Cc:Cc + 3], d(y_t)[rows]) and torch.equal(pre[:, Cc + 3:], d(sc)[rows])
    with pytest.raises(ValueError):                                   # an x without room for the third part
        ops.stack_views(d(y_cond), d(y_t), None, d(level), d(angle), off, S, x=pre[:S, :Cc + 3].contiguous(), self_cond=d(sc))
    with pytest.raises(ValueError):
        ops.stack_views(d(y_cond), d(y_t), None, d(level), d(angle), off, S, self_cond=d(sc)[:, :2].contiguous())


# ---- 2. ops: the coin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.25, 0.5, 1.0])
def test_draw_self_cond_is_the_host_mirror(dev, p):
    from view_fusion_amd import ops
    ids = torch.tensor(list(range(300)) + [2 ** 32 - 1, 2 ** 32, 2 ** 33 + 9, 2 ** 63 - 1])
    for seed in (0, SEED, 2 ** 64 - 1):
        got = ops.draw_self_cond(seed, ids.to(dev), p)
        assert got.dtype == torch.uint8 and torch.equal(got.cpu(), ops.self_cond_draw_host(seed, ids, p))
        assert np.array_equal(got.cpu().numpy().astype(bool), selfcond_ref.coin(seed, ids.numpy(), p))


# ---- 3. ops: the estimate ----------------------------------------------------------------------------------------------------
_EST = {}


def _est_inputs(shape):
    """Fixed-seed inputs of self_cond_estimate for one shape, made once and left unchanged."""
    if shape not in _EST:
        (H, W), vc = SHAPES[shape]
        B = len(vc)
        g = torch.Generator().manual_seed(61 + H)
        out = torch.randn(sum(vc), 6, H, W, generator=g) * 2
        y_t = torch.randn(B, 3, H, W, generator=g)
        y_cond = torch.rand(B, max(vc), 3, H, W, generator=g)
        _EST[shape] = (out, y_t, y_cond, vc)
    return _EST[shape]


@pytest.mark.parametrize("prediction", prediction_ref.PREDICTIONS)
@pytest.mark.parametrize("weighting", [True, False], ids=["softmax", "mean"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_self_cond_estimate_against_the_restatement(dev, shape, weighting, prediction):
    from view_fusion_amd import ops
    out, y_t, y_cond, vc = _est_inputs(shape)
    B, S = len(vc), sum(vc)
    n4 = 3 * out.shape[2] * out.shape[3] // 4
    assert (n4 < 256) if shape == "8x8" else (n4 > 64 * 256) if shape == "128x192" else (n4 % 256 != 0)
    gam = _gammas32()
    # levels near both ends of the schedule (B = 1: one run at each end)
    level_sets = [gam[[0, T // 2, T - 1]]] if B == 3 else [gam[[0]], gam[[T - 1]]]
    off, _, max_v = ops.view_offsets(list(vc), dev)
    for levels in level_sets:
        lv = torch.from_numpy(np.ascontiguousarray(levels)).to(dev)
        x, _, _ = ops.stack_views(y_cond.to(dev), y_t.to(dev), None, lv, torch.zeros(B, 1, device=dev), off, S, sc_channels=True)
        for keep in (None, torch.tensor([1, 0, 1][:B], dtype=torch.uint8) if B == 3 else torch.tensor([0], dtype=torch.uint8)):
            kd = None if keep is None else keep.to(dev)
            got = ops.self_cond_estimate(out.to(dev), off, lv, B, weighting, prediction, x=x, keep=kd)
            want = selfcond_ref.estimate(out.numpy(), vc, weighting, levels, prediction, y_t.numpy(),
                                         None if keep is None else keep.numpy())
            e = rel(got, want)
            print(f"{shape} {'softmax' if weighting else 'mean'} {prediction} levels {levels} keep {None if keep is None else keep.tolist()}: "
                  f"rel {e:.2e}  clamped share {float((got.abs() == 1).float().mean()):.2f}")
            assert torch.isfinite(got).all() and float(got.abs().max()) <= 1.0           # within [-1, 1] exactly
            assert e <= KERNEL_RTOL if float(np.abs(want).max()) > 0 else float(got.abs().max()) == 0.0
            if keep is not None:
                assert all(float(got[b].abs().max()) == 0.0 for b in range(B) if not keep[b])
            # y_t from a plain buffer: the same bits; a second call too (no atomics)
            if prediction != "x0":
                assert torch.equal(got, ops.self_cond_estimate(out.to(dev), off, lv, B, weighting, prediction, y_t=y_t.to(dev), keep=kd))
            assert torch.equal(got, ops.self_cond_estimate(out.to(dev), off, lv, B, weighting, prediction, x=x, keep=kd))
            if prediction == "x0" and weighting and keep is None:                        # clamp(compose) to the bit
                comp, _ = ops.compose(out.to(dev), off, B, max_v, True, want_weights=False)
                assert torch.equal(got, comp.clamp(-1.0, 1.0))
    with pytest.raises(ValueError):
        ops.self_cond_estimate(out.to(dev), off, lv, B, weighting, "eps")                 # neither x= nor y_t=
    with pytest.raises(ValueError):
        ops.self_cond_estimate(out.to(dev)[:, :3].contiguous(), off, lv, B, True, "eps", y_t=y_t.to(dev))


# ---- 4. model level ------------------------------------------------------------------------------------------------------
def _model(dev, Cc=3, prediction="eps", dropout=0, sched=SCHED):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**dict(WIDE[Cc], dropout=dropout))
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": dict(sched)}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    vf.set_prediction(prediction)
    return vf


def _batch(dev, B, vc, s=0, Cc=3):
    from view_fusion_amd import train
    b = dict(train.synthetic_batch(B, 3, 16, dev, seed=40 + s), view_count=torch.tensor(vc))
    if Cc == 6:
        b["y_cond"] = torch.rand(B, 3, 6, 16, 16, generator=torch.Generator().manual_seed(70 + s)).to(dev)
    return b


_ORACLE = {}


def _oracle(Cc):
    """The weights of _model and their CPU oracle, made once per stem width and left unchanged."""
    if Cc not in _ORACLE:
        from oracle import unet_ref
        from view_fusion_amd import UNet
        from view_fusion_amd.utils import deterministic_fill_
        net = UNet(**WIDE[Cc])
        deterministic_fill_(net.state_dict())
        sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
        _ORACLE[Cc] = dict(sd=sd, unet=lambda x, a, l: unet_ref.unet_forward(sd, WIDE[Cc], x, a, l))
    return _ORACLE[Cc]


def _draws(vf, dev, seed, ids):
    """The seeded draws of a training forward, from the library's own kernels (their parity is test_gpu_rng.py's)."""
    from view_fusion_amd import ops
    t, level, _ = ops.draw_train(seed, ids, vf.gammas)
    noise = ops.randn_ids(seed, ids, ops.diffusion.RNG_TRAIN_NOISE, 0, (3, 16, 16))
    return t, level, noise


@pytest.mark.parametrize("Cc", [3, 6])
def test_self_cond_targets_against_the_two_pass_chain(dev, Cc):
    from view_fusion_amd import ops
    vf = _model(dev, Cc)
    vf.set_self_cond(0.5)
    vf.train()
    batch, ids = _batch(dev, 3, VC, Cc=Cc), torch.tensor(IDS, device=dev)
    tgt = vf.self_cond_targets(batch["y_cond"], batch["view_count"], batch["angle"], batch["y_0"], seed=SEED, sample_ids=ids)
    keep, xh = vf.last_self_cond
    assert set(tgt) == {"self_cond"} and tgt["self_cond"] is xh
    host = ops.self_cond_draw_host(SEED, ids.cpu(), 0.5)
    assert keep.dtype == torch.uint8 and torch.equal(keep.cpu(), host) and 0 < int(host.sum()) < 3     # a mixed mask
    _, level, noise = _draws(vf, dev, SEED, ids)
    want, _ = selfcond_ref.first_pass(_oracle(Cc)["unet"], batch["y_cond"].cpu(), VC, batch["angle"].cpu(), batch["y_0"].cpu(),
                                      noise.cpu(), level.cpu(), "eps", True, host.numpy())
    e = maxabs(xh, want)
    print(f"Cc {Cc}: keep {host.tolist()}  x^ max-abs {e:.3e} against the float64 two-pass chain  |x^| max {float(xh.abs().max()):.4f}")
    assert e <= CHAIN_TOL and all(float(xh[b].abs().max()) == 0.0 for b in range(3) if not host[b])
    assert float(xh.abs().max()) > 0.1
    # unseeded: the draws come back, and the coin is drawn after them
    torch.manual_seed(5)
    tg2 = vf.self_cond_targets(batch["y_cond"], batch["view_count"], batch["angle"], batch["y_0"])
    assert set(tg2) == {"self_cond", "t", "u", "noise"}
    torch.manual_seed(5)
    t = torch.randint(1, T, (3,), device=dev).long()
    u = torch.rand((3, 1), device=dev)
    nz = torch.randn_like(batch["y_0"])
    kp = torch.rand(3, device=dev) < 0.5
    assert torch.equal(tg2["t"], t) and torch.equal(tg2["u"], u) and torch.equal(tg2["noise"], nz)
    assert torch.equal(vf.last_self_cond[0].bool(), kp)


CASES = {"eps": dict(prediction="eps"), "v-min_snr": dict(prediction="v", loss="min_snr"),
         "x0-cond_dropout": dict(prediction="x0", drop=0.5)}


@pytest.mark.parametrize("name", list(CASES))
def test_forward_against_the_oracles_second_pass(dev, name):
    """forward() against the oracle's second pass fed the device's own estimate: loss and every parameter gradient.
    Discrimination: against an oracle whose gradient flows through the first pass the same comparison misses."""
    from view_fusion_amd import ops
    case = CASES[name]
    pred = case["prediction"]
    vf = _model(dev, 3, pred)
    if case.get("loss"):
        vf.set_loss(weighting=case["loss"])
    if case.get("drop"):
        vf.set_cond_dropout(case["drop"])
    vf.set_self_cond(0.5)
    vf.train()
    batch, ids = _batch(dev, 3, VC), torch.tensor(IDS, device=dev)
    seen = []
    hook = vf.denoise_fn.register_forward_pre_hook(lambda m, a: seen.append(a[0].clone()))
    kw = dict(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"])
    loss = vf(**kw, seed=SEED, sample_ids=ids)
    hook.remove()
    loss.backward()
    keep, xh = vf.last_self_cond
    rows = torch.repeat_interleave(torch.arange(3), torch.tensor(VC)).to(dev)
    # what the UNet saw: zeros in pass 1, x^ in pass 2, bit for bit; the rest of the two inputs is the same
    assert len(seen) == 2 and float(seen[0][:, -3:].abs().max()) == 0.0 and torch.equal(seen[1][:, -3:], xh[rows])
    assert torch.equal(seen[0][:, :-3], seen[1][:, :-3])
    assert torch.equal(keep.cpu(), ops.self_cond_draw_host(SEED, ids.cpu(), 0.5))
    assert not xh.requires_grad
    _, level, noise = _draws(vf, dev, SEED, ids)
    drop = None
    if case.get("drop"):
        drop = guidance_ref.cond_drop(SEED, np.array(IDS), case["drop"])
        assert np.array_equal(vf.last_cond_drop.cpu().numpy().astype(bool), drop) and drop.any() and not drop.all()
    weight = None if not case.get("loss") else prediction_ref.weights(level.cpu().numpy(), pred, case["loss"], 5.0)
    orc = _oracle(3)
    from oracle import unet_ref
    host = [t.cpu() for t in (batch["y_cond"], batch["angle"], batch["y_0"], noise, level)]

    def oracle_grads(flow):
        sd = {k: v.clone().requires_grad_(True) for k, v in orc["sd"].items()}
        fn = lambda x, a, l: unet_ref.unet_forward(sd, WIDE[3], x, a, l)                 # noqa: E731
        sc = xh.cpu()
        if flow:
            sc = selfcond_ref.flowing_estimate(fn, host[0], VC, host[1], host[2], host[3], host[4], pred, True,
                                               keep.cpu().numpy(), drop)
        ref = selfcond_ref.second_pass_loss(fn, host[0], VC, host[1], host[2], host[3], host[4], pred, sc, True, weight, drop)
        ref.backward()
        return float(ref.detach()), sd

    ref, sd = oracle_grads(False)
    _, sd_flow = oracle_grads(True)
    got = dict(vf.denoise_fn.named_parameters())
    miss = {k: grad_miss(got[k].grad, sd[k].grad) for k in got}
    miss_flow = {k: grad_miss(got[k].grad, sd_flow[k].grad) for k in got}
    worst, worst_flow = max(miss, key=miss.get), max(miss_flow, key=miss_flow.get)
    print(f"{name}: loss {float(loss.detach()):.9g}  oracle {ref:.9g}  rel {abs(float(loss.detach()) - ref) / abs(ref):.2e}; "
          f"gradients: worst {miss[worst]:.3f} of the tolerance ({worst}); against a gradient that flows through pass 1: "
          f"{miss_flow[worst_flow]:.1f} of the tolerance ({worst_flow}), {sum(v > 1 for v in miss_flow.values())} of "
          f"{len(miss_flow)} parameters miss")
    assert close(float(loss.detach()), ref)
    assert max(miss.values()) <= 1.0
    assert max(miss_flow.values()) > 1.0                       # a flowing gradient would not pass
    # an injected estimate reproduces the loss bit for bit and runs no first pass
    seen.clear()
    hook = vf.denoise_fn.register_forward_pre_hook(lambda m, a: seen.append(1))
    loss_i = vf(**kw, seed=SEED, sample_ids=ids, self_cond=xh)
    hook.remove()
    assert torch.equal(loss_i.detach(), loss.detach()) and len(seen) == 1
    # eval mode keeps every sample and draws nothing
    vf.eval()
    state = torch.cuda.get_rng_state(dev)
    vf(**kw, seed=SEED, sample_ids=ids)
    assert torch.equal(vf.last_self_cond[0], torch.ones(3, dtype=torch.uint8, device=dev))
    assert torch.equal(torch.cuda.get_rng_state(dev), state)


def test_the_first_pass_applies_no_dropout(dev):
    vf = _model(dev, 3, dropout=0.2)
    vf.set_self_cond(1.0)
    batch, ids = _batch(dev, 3, VC), torch.tensor(IDS, device=dev)
    args = (batch["y_cond"], batch["view_count"], batch["angle"], batch["y_0"])
    vf.train()
    a = vf.self_cond_targets(*args, seed=SEED, sample_ids=ids)["self_cond"]
    assert vf.denoise_fn.training and torch.equal(vf.last_self_cond[0], torch.ones(3, dtype=torch.uint8, device=dev))
    b = vf.self_cond_targets(*args, seed=SEED, sample_ids=ids)["self_cond"]
    vf.eval()
    c = vf.self_cond_targets(*args, seed=SEED, sample_ids=ids)["self_cond"]
    assert torch.equal(a, b) and torch.equal(a, c) and float(a.abs().max()) > 0.1
    # ... while the second pass does: two training forwards without a seed differ
    vf.train()
    inj = dict(t=torch.tensor([15, 3, 9], device=dev), u=torch.full((3, 1), 0.5, device=dev), noise=torch.randn_like(batch["y_0"]))
    kw = dict(y_cond=args[0], view_count=args[1], angle=args[2], y_0=args[3], self_cond=a, **inj)
    assert not torch.equal(vf(**kw).detach(), vf(**kw).detach())
    # p = 0: no first pass at all, zeros are stacked
    vf.set_self_cond(0.0)
    calls = []
    hook = vf.denoise_fn.register_forward_pre_hook(lambda m, x: calls.append(x[0][:, -3:].clone()))
    vf(y_cond=args[0], view_count=args[1], angle=args[2], y_0=args[3], seed=SEED, sample_ids=ids)
    hook.remove()
    assert len(calls) == 1 and float(calls[0].abs().max()) == 0.0 and vf.last_self_cond[1] is None


# ---- 5. sampling ------------------------------------------------------------------------------------------------------------
K = 4
SAMPLERS = {"ddim": dict(solver="ddim", eta=0.5), "dpmpp2m": dict(solver="dpmpp2m", eta=0.0)}


def _gen(vf, batch, ids, **kw):
    return vf.generate(batch["y_cond"], batch["view_count"], batch["angle"], seed=SEED, sample_ids=ids, **kw)[0]


def _ref_chain(dev, batch, ids, solver, eta, guidance=None, tau=None, **kw):
    from view_fusion_amd import ops
    tau = sampler_ref.timesteps(T, K) if tau is None else tau
    y_T = ops.randn_ids(SEED, ids, ops.diffusion.RNG_START_NOISE, 0, (3, 16, 16)).cpu()
    z_seq = None
    if eta:
        z_seq = torch.zeros(T, 3, 3, 16, 16)
        for t in tau:
            z_seq[int(t)] = ops.randn_ids(SEED, ids, ops.diffusion.RNG_STEP_NOISE, int(t), (3, 16, 16)).cpu()
    return selfcond_ref.chain(_oracle(3)["unet"], _betas(), "eps", batch["y_cond"].cpu(), VC, batch["angle"].cpu(), y_T, z_seq,
                              tau, solver, eta, g=guidance, **kw)


@pytest.mark.parametrize("guidance", [None, 2.0], ids=["plain", "guided"])
@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_generate_against_the_self_conditioned_chain(dev, sampler, guidance, monkeypatch):
    vf = _model(dev)
    vf.set_self_cond(0.5)
    vf.eval()
    batch, ids = _batch(dev, 3, VC), torch.tensor(IDS, device=dev)
    kw = dict(sample_steps=K, guidance=guidance, **SAMPLERS[sampler])
    eager = _gen(vf, batch, ids, use_graph=False, **kw)
    states, _ = _ref_chain(dev, batch, ids, guidance=guidance, **SAMPLERS[sampler])
    cut, _ = _ref_chain(dev, batch, ids, guidance=guidance, force_zero=True, **SAMPLERS[sampler])
    e, live = maxabs(eager, states[-1]), maxabs(eager, cut[-1])
    print(f"{sampler} {'guided' if guidance else 'plain'}: max-abs {e:.3e} against the float64 chain; "
          f"{live:.3e} from the chain with the estimate forced to zero")
    assert e <= CHAIN_TOL
    assert live > 10 * CHAIN_TOL                                             # the wire is live
    assert torch.equal(_gen(vf, batch, ids, use_graph=True, **kw), eager)    # graph replay is bitwise eager
    # zero initialisation: a history buffer that arrives full of garbage changes nothing
    made = []
    monkeypatch.setattr(vf, "_history_buffer", lambda y: made.append(torch.full_like(y, float("nan"))) or made[-1])
    assert torch.equal(_gen(vf, batch, ids, use_graph=False, **kw), eager)
    assert torch.equal(_gen(vf, batch, ids, use_graph=True, **kw), eager)
    assert len(made) == 2 and all(torch.isfinite(h).all() for h in made)


def test_the_default_chain_of_a_self_conditioned_model(dev):
    vf = _model(dev)
    vf.set_self_cond(0.5)
    vf.eval()
    batch, ids = _batch(dev, 3, VC), torch.tensor(IDS, device=dev)
    a = vf.generate(batch["y_cond"], batch["view_count"], batch["angle"], seed=SEED, sample_ids=ids)
    b = vf.generate(batch["y_cond"], batch["view_count"], batch["angle"], seed=SEED, sample_ids=ids, sample_steps=T,
                    solver="ddim", eta=1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(a[0]).all()
    # one reverse step by hand: None is zeros
    y = torch.randn(3, 3, 16, 16, device=dev)
    t = torch.full((3,), 7, device=dev)
    z = torch.randn_like(y)
    args = (y, batch["y_cond"], batch["view_count"], batch["angle"], t)
    none, zeros = vf.p_sample(*args, z=z)[0], vf.p_sample(*args, z=z, self_cond=torch.zeros_like(y))[0]
    fed = vf.p_sample(*args, z=z, self_cond=y.clamp(-1, 1))[0]
    assert torch.equal(none, zeros) and not torch.equal(none, fed)
    m0 = vf.p_mean_variance(*args, True)[0]
    assert torch.equal(m0, vf.p_mean_variance(*args, True, self_cond=torch.zeros_like(y))[0])


def test_a_thresholded_step_feeds_back_the_thresholded_y0(dev, monkeypatch):
    from view_fusion_amd import ops
    vf = _model(dev)
    vf.set_self_cond(0.5)
    vf.eval()
    batch, ids = _batch(dev, 3, VC), torch.tensor(IDS, device=dev)
    wrote, fed = [], []
    real = ops.sampler_step

    def spy(*a, **k):
        r = real(*a, **k)
        wrote.append(k["y0_prev"].clone())
        return r

    monkeypatch.setattr(ops, "sampler_step", spy)
    hook = vf.denoise_fn.register_forward_pre_hook(lambda m, a: fed.append(a[0][:3 + 3, -3:].clone()))
    y = _gen(vf, batch, ids, use_graph=False, sample_steps=K, solver="dpmpp2m", guidance=2.0, threshold=0.9)
    hook.remove()
    rows = torch.repeat_interleave(torch.arange(3), torch.tensor(VC)).to(dev)
    assert len(wrote) == K and len(fed) == K and torch.isfinite(y).all()
    assert float(fed[0].abs().max()) == 0.0
    for k in range(1, K):                                    # bitwise the buffer the tail wrote
        assert torch.equal(fed[k], wrote[k - 1][rows])
    _, y0s = _ref_chain(dev, batch, ids, "dpmpp2m", 0.0, guidance=2.0, q=0.9)
    errs = [maxabs(w, r) for w, r in zip(wrote, y0s)]
    plain = [maxabs(w, r) for w, r in zip(wrote, _ref_chain(dev, batch, ids, "dpmpp2m", 0.0, guidance=2.0)[1])]
    print(f"thresholded y0 against the float64 chain, per step: {['%.2e' % e for e in errs]}; against the statically clamped "
          f"chain: {['%.2e' % e for e in plain]}")
    assert max(errs) <= CHAIN_TOL and all(float(w.abs().max()) <= 1.0 for w in wrote)


# ---- 6. Trainer --------------------------------------------------------------------------------------------------------------
TB, TVC, TSEED = 4, [1, 3, 2, 2], 11


def _trainer(dev, graph, seed=TSEED, **kw):
    from view_fusion_amd import train
    vf = _model(dev)
    vf.set_self_cond(0.5)
    tr = train.Trainer(vf, lr_warmup=1, graph=graph, seed=seed, **kw)
    tr.it = 0
    return vf, tr


def _steps(dev, vf, tr, n, first=0):
    out = []
    for s in range(first, first + n):
        loss = tr.step(_batch(dev, TB, TVC, s)).clone()
        out.append((loss, vf.last_self_cond[0].clone(), vf.last_self_cond[1].clone()))
    return out


def _same(a, b):
    return all(torch.equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def test_trainer_graph_replay_equals_eager(dev):
    from view_fusion_amd import ops, train
    (vf_e, tr_e), (vf_g, tr_g) = _trainer(dev, False), _trainer(dev, True)
    re_, rg = _steps(dev, vf_e, tr_e, 4), _steps(dev, vf_g, tr_g, 4)
    assert tr_e.graph_steps == 0 and tr_g.graph_steps == 2 and tr_g.mode == "graph"
    assert _same(re_, rg)
    assert all(torch.equal(p, q) for p, q in zip(vf_e.parameters(), vf_g.parameters()))
    assert len({float(r[0]) for r in rg}) == 4
    masks = torch.stack([r[1] for r in rg]).cpu()
    for it, m in enumerate(masks, start=1):                  # a sample's coin is a function of (seed, id)
        first = train.step_sample_ids(it, TB)
        assert torch.equal(m, ops.self_cond_draw_host(TSEED, torch.arange(first, first + TB), 0.5))
    assert 0 < int(masks.sum()) < masks.numel()
    # set_self_cond(None) after the capture: the captured steps are dropped and the plain step runs -- the 9-channel stem
    # then takes a `relative` batch (6 conditioning channels + the target)
    plain = _model(dev)
    plain.load_state_dict(vf_g.state_dict())
    tr_p = train.Trainer(plain, lr_warmup=1, graph=False, seed=TSEED)
    tr_p.it = tr_g.it
    for m in (vf_e, vf_g):
        m.set_self_cond(None)
    n = tr_g.graph_steps
    bt = _batch(dev, TB, TVC, 9, Cc=6)
    le, lg, lp = tr_e.step(bt), tr_g.step(bt), tr_p.step(bt)
    assert tr_g.graph_steps == n and vf_g.last_self_cond is None
    assert torch.equal(le, lg) and torch.equal(lg, lp)
    assert all(torch.equal(p, q) for p, q in zip(vf_e.parameters(), vf_g.parameters()))


def test_trainer_unseeded_with_the_phases_draws_injected(dev):
    (vf_e, tr_e), (vf_g, tr_g) = _trainer(dev, False, seed=None), _trainer(dev, True, seed=None)
    torch.manual_seed(77)
    re_ = _steps(dev, vf_e, tr_e, 4)
    torch.manual_seed(77)
    rg = _steps(dev, vf_g, tr_g, 4)
    assert tr_g.graph_steps == 2 and _same(re_, rg)
    assert all(torch.equal(p, q) for p, q in zip(vf_e.parameters(), vf_g.parameters()))


def test_trainer_accum_steps(dev):
    (vf_e, tr_e), (vf_g, tr_g) = _trainer(dev, False, accum_steps=2), _trainer(dev, True, accum_steps=2)
    (vf_1, tr_1) = _trainer(dev, False)
    re_, rg, r1 = _steps(dev, vf_e, tr_e, 3), _steps(dev, vf_g, tr_g, 3), _steps(dev, vf_1, tr_1, 3)
    assert tr_g.graph_steps >= 1 and _same(re_, rg)
    assert all(torch.equal(p, q) for p, q in zip(vf_e.parameters(), vf_g.parameters()))
    # the last micro-batch holds samples 2, 3 of the undivided batch: the same coins; the estimate went through the UNet
    # in another batch (another split of the same sums), so it and the loss are compared at the chain tolerance
    assert vf_g.last_self_cond[0].numel() == TB // 2
    assert torch.equal(rg[0][1], r1[0][1][TB // 2:])
    ex = float((rg[0][2] - r1[0][2][TB // 2:]).abs().max())
    el = abs(float(rg[0][0]) - float(r1[0][0])) / abs(float(r1[0][0]))
    print(f"accum_steps 2 against the undivided batch, step 0: x^ max-abs {ex:.3e}  loss rel {el:.3e}")
    assert ex <= CHAIN_TOL and el <= CHAIN_TOL


# ---- 7. defaults untouched -----------------------------------------------------------------------------------------------------
def _plain(dev):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": dict(SCHED)}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


def test_the_default_step_is_untouched(dev):
    from view_fusion_amd import ops
    B = 3
    batch = _batch(dev, B, VC)
    g = torch.Generator().manual_seed(1)
    inj = dict(t=torch.tensor([15, 3, 9]).to(dev), u=torch.rand(B, 1, generator=g).to(dev),
               noise=torch.randn(B, 3, 16, 16, generator=g).to(dev))
    runs = []
    for touch in ("never", "none", "set-unset"):
        vf = _plain(dev)
        if touch == "none":
            vf.set_self_cond(None)
        elif touch == "set-unset":
            vf.set_self_cond(0.5)
            vf.set_self_cond(None)
        vf.train()
        ops.st.KERNEL_LOG = []
        try:
            loss = vf(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"], **inj)
            loss.backward()
            names = [r[5] for r in ops.st.KERNEL_LOG]
        finally:
            ops.st.KERNEL_LOG = None
        assert vf.last_self_cond is None and vf.self_cond is None
        runs.append((loss.detach().cpu(), [p.grad.cpu() for p in vf.parameters()], names))
    for lb, gb, nb in runs[1:]:
        assert torch.equal(runs[0][0], lb) and all(torch.equal(x, y) for x, y in zip(runs[0][1], gb)) and nb == runs[0][2]
    names = runs[0][2]
    assert not [n for n in names if n in NEW or "_sc" in n or "self_cond" in n]
    glue = [n for n in names if n in ("vf_gather_level", "vf_stack_views", "vf_stack_views_cfg", "vf_compose_fwd",
                                      "vf_compose_mse_bwd", "vf_draw_train", "vf_randn_ids")]
    assert glue == ["vf_gather_level", "vf_stack_views", "vf_compose_fwd", "vf_compose_mse_bwd"]


def test_a_default_generate_allocates_its_history_only_under_dpmpp2m(dev, monkeypatch):
    from view_fusion_amd import ops
    vf = _plain(dev)
    vf.eval()
    batch = _batch(dev, 3, VC)
    made = []
    monkeypatch.setattr(vf, "_history_buffer", lambda y: made.append(1) or torch.empty_like(y))
    counts, logs = {}, {}
    for name, kw in (("ancestral", {}), ("ddim", dict(sample_steps=3)), ("dpmpp2m", dict(sample_steps=3, solver="dpmpp2m"))):
        del made[:]
        ops.st.KERNEL_LOG = []
        try:
            vf.generate(batch["y_cond"], batch["view_count"], batch["angle"], seed=SEED, use_graph=False, **kw)
            logs[name] = [r[5] for r in ops.st.KERNEL_LOG]
        finally:
            ops.st.KERNEL_LOG = None
        counts[name] = len(made)
    assert counts == dict(ancestral=0, ddim=0, dpmpp2m=1)
    assert not [n for names in logs.values() for n in names if n in NEW or "_sc" in n or "self_cond" in n]
    assert logs["ancestral"].count("vf_p_sample_tail_rng") == T and logs["ancestral"].count("vf_stack_views") == T + 1
    # on a self-conditioned model the sibling kernel takes every stacking launch, and nothing else changes name
    sc = _model(dev)
    sc.set_self_cond(0.5)
    sc.eval()
    ops.st.KERNEL_LOG = []
    try:
        sc.generate(batch["y_cond"], batch["view_count"], batch["angle"], seed=SEED, use_graph=False, sample_steps=3)
        on = [r[5] for r in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None
    assert on.count("vf_stack_views_sc") == 4 and "vf_stack_views" not in on and "vf_stack_views_cfg" not in on
    assert on.count("vf_sampler_step") == logs["ddim"].count("vf_sampler_step") == 3
