"""The analytic variance at model level on the GPU (ViewFusion.eps_moments / set_moments, generate(variance="analytic"),
bound_terms(fixed_variance="analytic"), drivers.estimate_moments; definition at the head of csrc/diffusion.hip) -- the
TINY UNet on 8 x 8 images, the T = 20 linear 1e-4 ... 0.09 schedule of the bound's kernel tests, view counts (3, 2).

  1. wiring: eps_moments is tests/analytic_ref.py fed the device's own UNet outputs (a forward hook), level by level, for
     eps / v / x0 on the full chain and on five levels.  Tolerance: the kernel tolerance of tests/test_gpu_analytic.py --
     4 x the float32 restatement's own distance from float64 over the chain's levels (every measured floor is nonzero).
     A seeded run shows a sample the same noisy targets, bit for bit, whatever batch it stands in, and its moments are
     the same bits too: through a network that treats rows independently (the Gaussian one below) by construction, and
     through this UNet at these row counts (1, 2, 3 and 5 stacked rows) as measured -- nothing in the feature's own
     launches depends on the batch.
  2. generate(variance="analytic") with every moment = 1 is generate() without it, bit for bit (eta = 1 and 0.5, K = 5,
     seeded); variance=None logs the launches of before; the analytic chain logs the launches of the same chain with the
     fixed row, and Analytic-DDIM (eta = 0) draws noise where DDIM draws none.
  3. with moments in (0, 1) and an injected z_seq the K = 5 chain is tests/sampler_ref.py's step on the analytic sigma row
     through the oracle UNet, within the chain tolerance tests/test_gpu_sampler_steps.py gives the same chain with the
     fixed row (max-abs 1e-3).
  4. optimality on Gaussian data: with the exact noise estimate of N(0, s^2) targets as the network, the estimated
     moments make sum_{k >= 1} vb of the K = 5 chain smaller than 0.9 x the better of "small" and "large" (a float64
     simulation of this setup over 30 seeds gave worst ratios 0.77 and 0.68).
  5. drivers.estimate_moments, the checkpoint round trip, the drivers that forward variance=, the refusals.
Figures are printed before the assertions (run with -s); profiles/analytic_variance.md records them."""
import numpy as np
import pytest
import torch

import analytic_ref
import sampler_ref
from conftest import TINY

pytestmark = pytest.mark.gpu
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
T = SCHED["num_timesteps"]
VC = [3, 2]
B, HW = 2, (8, 8)
CHAIN_TOL = 1e-3                                                     # tests/test_gpu_sampler_steps.py, max-abs


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _model(dev, cfg=TINY, sched=SCHED, prediction="eps"):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**cfg)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": dict(sched)}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    vf.set_prediction(prediction)
    return vf


@pytest.fixture(scope="module")
def vf(dev):
    return _model(dev)


@pytest.fixture(scope="module")
def batch(dev):
    g = torch.Generator().manual_seed(4)
    y_0 = torch.rand(B, 3, *HW, generator=g) * 2 - 1
    y_cond = torch.rand(B, max(VC), 3, *HW, generator=g) * 2 - 1
    angle = 2 * np.pi / 24 * torch.randint(0, 24, (B, 1), generator=g).float()
    noise = torch.randn(B, T, 3, *HW, generator=g)
    c = dict(y_0=y_0, y_cond=y_cond, angle=angle, noise=noise, y_T=torch.randn(B, 3, *HW, generator=g),
             z_seq=torch.randn(T, B, 3, *HW, generator=g))
    c["gpu"] = {k: v.to(dev) for k, v in c.items()}
    return c


def _hooked(vf, fn):
    """fn() with every (input, output) of the network kept, in call order."""
    calls = []
    h = vf.denoise_fn.register_forward_hook(lambda m, i, o: calls.append((i[0].detach().clone(), o.detach().clone())))
    try:
        return fn(), calls
    finally:
        h.remove()


def _rel(a, b):
    return float((np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)).max())


def _wiring(vf, batch, dev, levels):
    """eps_moments with injected noise against the restatement on the network's own outputs
    -> (the result, [(k, device rel error, float32 restatement's rel error)])."""
    from view_fusion_amd import ops, schedule
    g = batch["gpu"]
    tau = np.arange(T) if levels is None else schedule.sample_timesteps(T, levels)
    K = len(tau)
    noise = g["noise"][:, :K].contiguous()
    res, calls = _hooked(vf, lambda: vf.eps_moments(g["y_cond"], VC, g["angle"], g["y_0"], noise=noise, levels=levels))
    assert len(calls) == K and res["tau"].tolist() == tau.tolist() and tuple(res["m2"].shape) == (B, K)
    tab = {k: v.astype(np.float32) for k, v in schedule.eps_tables(vf.betas64, tau, vf.prediction).items()}
    tau_d = torch.from_numpy(tau.astype(np.int64)).to(dev)
    rec = []
    for k in range(K):
        x, out = calls[K - 1 - k]                                    # the loop runs k = K-1 ... 0
        kidx = torch.full((B,), k, device=dev, dtype=torch.int64)
        y_k = ops.nll_noisy(g["y_0"], kidx, tau_d, vf.gammas, noise=noise)
        assert torch.equal(x[0, 3:6], y_k[0]) and torch.equal(x[VC[0], 3:6], y_k[1])     # what the network was shown
        args = (out.cpu().numpy(), VC, True, y_k.cpu().numpy(), tab["ea"][k], tab["eb"][k])
        r64, r32 = analytic_ref.moment(*args), analytic_ref.moment(*args, dt=np.float32)
        rec.append((k, _rel(res["m2"][:, k].cpu().numpy(), r64), _rel(r32, r64)))
    return res, rec


# ---- 1. wiring -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [None, 5])
@pytest.mark.parametrize("prediction", ["eps", "v", "x0"])
def test_eps_moments_is_the_restatement_on_the_devices_own_outputs(dev, batch, prediction, levels):
    vf = _model(dev, prediction=prediction)
    res, rec = _wiring(vf, batch, dev, levels)
    floor = max(r[2] for r in rec)
    print(f"{prediction} levels={levels}: fp32 restatement floor {floor:.2e}, device worst {max(r[1] for r in rec):.2e}; "
          f"m2 {res['m2'][0].cpu().numpy()}")
    assert floor > 0 and all(r[1] <= 4.0 * floor for r in rec), rec
    assert torch.isfinite(res["m2"]).all() and (res["m2"] > 0).all()


def test_nine_channels_and_training_mode(dev, batch):
    """Channels 6..8 of a nine-channel network are ignored; the network runs on its inference path and is left in the
    mode it was in."""
    g = batch["gpu"]
    nine = _model(dev, dict(TINY, out_channel=9, dropout=0.2))
    nine.train()
    res, rec = _wiring(nine, batch, dev, 5)
    assert nine.training and nine.denoise_fn.training
    floor = max(r[2] for r in rec)
    assert floor > 0 and all(r[1] <= 4.0 * floor for r in rec), rec
    again = nine.eps_moments(g["y_cond"], VC, g["angle"], g["y_0"], noise=g["noise"][:, :5].contiguous(), levels=5)
    assert torch.equal(res["m2"], again["m2"])                        # no Dropout, the same bits on every run


def _targets_shown(vf, fn, counts):
    res, calls = _hooked(vf, fn)
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    return res, [x[first.tolist(), 3:6].cpu().numpy() for x, _ in calls]


def test_seeded_moments_do_not_depend_on_the_batch(dev, vf, batch):
    g = batch["gpu"]
    args = lambda rows: (g["y_cond"][rows], [VC[i] for i in rows], g["angle"][rows], g["y_0"][rows])    # noqa: E731
    ids = [7, 3]
    both, shown = _targets_shown(vf, lambda: vf.eps_moments(*args([0, 1]), seed=5, sample_ids=ids), VC)
    again = vf.eps_moments(*args([0, 1]), seed=5, sample_ids=ids)
    other = vf.eps_moments(*args([0, 1]), seed=6, sample_ids=ids)
    assert torch.equal(both["m2"], again["m2"]) and not torch.equal(both["m2"], other["m2"])
    _, rec = _wiring(vf, batch, dev, None)
    tol = 4.0 * max(r[2] for r in rec)
    for i in (1, 0):
        alone, shown_i = _targets_shown(vf, lambda: vf.eps_moments(*args([i]), seed=5, sample_ids=ids[i:i + 1]), [VC[i]])
        for j in range(T):                                            # the same noisy targets, bit for bit
            assert np.array_equal(shown[j][i], shown_i[j][0])
        e = _rel(alone["m2"][0].cpu().numpy(), both["m2"][i].double().cpu().numpy())
        print(f"sample {i} alone against the batch of two through the UNet: rel {e:.2e} (tolerance {tol:.2e}), same bits: "
              f"{torch.equal(alone['m2'][0], both['m2'][i])}")
        assert e <= tol
        assert torch.equal(alone["m2"][0], both["m2"][i])             # measured: this UNet's rows are the same bits here
    assert torch.isfinite(vf.eps_moments(*args([0, 1]))["m2"]).all()   # torch's device generator runs too


# ---- 2. moments = 1, variance=None, launches ----------------------------------------------------------------------------------------
def _gen(vf, batch, **kw):
    g = batch["gpu"]
    return vf.generate(g["y_cond"], VC, g["angle"], **kw)


def _names(vf, batch, **kw):
    from view_fusion_amd import ops
    try:
        ops.st.KERNEL_LOG = []
        _gen(vf, batch, use_graph=False, **kw)
        return [e[5] for e in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None


@pytest.mark.parametrize("eta", [1.0, 0.5])
def test_moments_of_one_give_the_fixed_row_bit_for_bit(vf, batch, eta):
    kw = dict(sample_steps=5, solver="ddim", eta=eta, seed=11, sample_ids=[4, 9])
    vf.set_moments(None)
    plain = _gen(vf, batch, **kw)
    vf.set_moments(np.ones(T))
    same = _gen(vf, batch, variance="analytic", **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, same))
    assert all(torch.equal(a, b) for a, b in zip(plain, _gen(vf, batch, variance=None, **kw)))
    assert all(torch.equal(a, b) for a, b in zip(plain, _gen(vf, batch, variance="analytic", use_graph=False, **kw)))
    vf.set_moments(np.full(T, 0.5))                                  # the plan follows the moments
    other = _gen(vf, batch, variance="analytic", **kw)
    assert not torch.equal(other[4], plain[4]) and torch.isfinite(other[1]).all()
    assert all(torch.equal(a, b) for a, b in zip(plain, _gen(vf, batch, **kw)))
    vf.set_moments(None)


def test_launches(vf, batch):
    g = batch["gpu"]
    kw = dict(sample_steps=5, seed=3)
    vf.set_moments(None)
    _gen(vf, batch, use_graph=False, **kw)                            # (the first call may pack weights)
    before = {eta: _names(vf, batch, eta=eta, **kw) for eta in (0.0, 0.5)}
    full = _names(vf, batch, seed=3)
    vf.set_moments(np.full(T, 0.5))
    for eta in (0.0, 0.5):                                           # variance=None: the launches of before
        assert _names(vf, batch, eta=eta, variance=None, **kw) == before[eta]
    assert _names(vf, batch, seed=3) == full and full.count("vf_p_sample_tail_rng") == T
    # the analytic chain: the launches of the chain with the fixed row -- only a table row differs
    assert _names(vf, batch, eta=0.5, variance="analytic", **kw) == before[0.5]
    assert before[0.5].count("vf_sampler_step_rng") == 5
    # Analytic-DDIM is stochastic: eta = 0 draws noise where DDIM draws none
    addim = _names(vf, batch, eta=0.0, variance="analytic", **kw)
    assert before[0.0].count("vf_sampler_step") == 5 and addim.count("vf_sampler_step_rng") == 5
    a = _gen(vf, batch, eta=0.0, variance="analytic", **kw)
    b = _gen(vf, batch, eta=0.0, variance="analytic", sample_steps=5, seed=4)
    assert not torch.equal(a[4], b[4])
    # sample_steps=None runs as sample_steps=T, "ddim", eta = 1 through the table-driven tail
    whole = _names(vf, batch, seed=3, variance="analytic")
    assert whole.count("vf_sampler_step_rng") == T and "vf_p_sample_tail_rng" not in whole
    c = _gen(vf, batch, seed=3, variance="analytic")
    d = _gen(vf, batch, seed=3, variance="analytic", sample_steps=T, solver="ddim", eta=1.0)
    assert all(torch.equal(x, y) for x, y in zip(c, d))
    # forward(generate=True) and p_sample take it too
    e = vf(g["y_cond"], VC, g["angle"], generate=True, seed=3, variance="analytic")
    assert all(torch.equal(x, y) for x, y in zip(c, e))
    t = torch.full((B,), 7, device=g["y_T"].device, dtype=torch.long)
    z = g["z_seq"][7]
    y_a, _, w_a = vf.p_sample(g["y_T"], g["y_cond"], VC, g["angle"], t, z=z, variance="analytic")
    y_p, _, w_p = vf.p_sample(g["y_T"], g["y_cond"], VC, g["angle"], t, z=z)
    y_m, _, _ = vf.p_sample(g["y_T"], g["y_cond"], VC, g["angle"], t, z=torch.zeros_like(z))
    plan = vf._sampler_plan(list(range(T)), "ddim", 1.0, z.device, "analytic")
    fixed = float(torch.exp(0.5 * vf.posterior_log_variance_clipped[7]))
    ratio = (y_a - y_m).norm() / (y_p - y_m).norm()                  # the same mean, another noise scale
    print(f"p_sample at t = 7: noise scale analytic / posterior {float(ratio):.6f}, tables {float(plan['sigma'][7]) / fixed:.6f}")
    assert torch.equal(w_a, w_p) and abs(float(ratio) - float(plan["sigma"][7]) / fixed) <= 1e-3 * float(ratio)
    vf.set_moments(None)


# ---- 3. the chain against the restatement on the analytic row ---------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_chain_against_the_oracle_on_the_analytic_row(vf, batch, eta):
    from oracle import unet_ref, view_fusion_ref as vfr
    g = batch["gpu"]
    K = 5
    M = np.random.default_rng(8).uniform(0.1, 0.9, T)
    vf.set_moments(M)
    y, ret, _, weights, samples = _gen(vf, batch, y_t=g["y_T"], z_seq=g["z_seq"], sample_steps=K, solver="ddim", eta=eta,
                                       variance="analytic")
    vf.set_moments(None)
    sd = {k: v.detach().cpu().clone() for k, v in vf.denoise_fn.state_dict().items()}
    betas = vfr.beta_schedule(**SCHED)
    gammas32 = vfr.schedule_buffers(betas)["gammas"]
    tau = sampler_ref.timesteps(T, K)
    sig = np.sqrt(analytic_ref.sigma2(betas, tau, M, eta))
    sig[0] = 0.0
    vc = torch.tensor(VC)
    state = batch["y_T"].double().numpy()
    states, w_ref = [], []
    with torch.no_grad():
        for k in reversed(range(K)):
            level = gammas32[int(tau[k])].reshape(1, 1).repeat(B, 1)
            x, ang_s, lvl_s = vfr.stack_views(batch["y_cond"], vc, torch.tensor(state).float(), level, batch["angle"])
            eps, _, w = vfr.compose(unet_ref.unet_forward(sd, TINY, x, ang_s, lvl_s), vc, True)
            mean, _ = sampler_ref.step(betas, tau, "ddim", eta, k, state, eps.double().numpy(), None, 0.0)
            state = mean + sig[k] * batch["z_seq"][int(tau[k])].double().numpy()
            states.append(torch.tensor(state).float())
            w_ref.append(w)
    err = float((ret[:, 1:].cpu() - torch.stack(states).transpose(0, 1)).abs().max())
    werr = float((weights.cpu() - torch.stack(w_ref, dim=1)).abs().max())
    plain = _gen(vf, batch, y_t=g["y_T"], z_seq=g["z_seq"], sample_steps=K, solver="ddim", eta=eta)
    away = float((plain[1] - ret).abs().max())
    print(f"analytic row, ddim eta {eta} K {K}: chain max-abs {err:.3e}  weights {werr:.3e}; from the fixed row's chain "
          f"{away:.3e}")
    assert ret.shape == (B, 1 + K, 3, *HW) and torch.equal(ret[:, 0], g["y_T"]) and torch.equal(samples, ret[:, -1])
    assert err <= CHAIN_TOL and werr <= CHAIN_TOL
    assert away > 10 * CHAIN_TOL                                      # the row matters
    assert samples.abs().max() <= 1.0                                 # the last step lands on the clamped y0


# ---- 4. optimality on Gaussian data ---------------------------------------------------------------------------------------------------
S2 = 0.05


def _gaussian_model(dev):
    """The exact noise estimate of targets drawn from N(0, S2): sqrt(1 - g) y_t / (g S2 + 1 - g) in channels 0..2, zero
    logits -- a foreign denoise_fn(x, angle, level) whose rows do not see one another."""
    from view_fusion_amd import ViewFusion

    def denoise_fn(x, angle, level):
        lv = level.reshape(-1, 1, 1, 1)
        out = torch.zeros(x.shape[0], 6, *x.shape[-2:], device=x.device, dtype=torch.float32)
        out[:, 0:3] = torch.sqrt(1.0 - lv) * x[:, 3:6] / (lv * S2 + 1.0 - lv)
        return out

    vf = ViewFusion(denoise_fn, {"train": dict(SCHED)}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


@pytest.fixture(scope="module")
def gaussian(dev):
    g = torch.Generator().manual_seed(12)
    n = 4
    y_0 = (S2 ** 0.5 * torch.randn(n, 3, *HW, generator=g)).to(dev)
    return dict(vf=_gaussian_model(dev), target=y_0, cond=torch.zeros(n, 1, 3, *HW, device=dev),
                angle=torch.zeros(n, 1, device=dev), view_count=[1] * n, ids=torch.arange(n))


def test_analytic_variance_is_better_on_gaussian_data(gaussian):
    from view_fusion_amd import drivers, schedule
    vf = gaussian["vf"]
    data = [{k: v for k, v in gaussian.items() if k != "vf"}]
    est = drivers.estimate_moments(vf, data, seed=1, levels=5)
    tau = schedule.sample_timesteps(T, 5)
    exact = analytic_ref.gaussian_moment(vf.betas64, S2)
    print(f"estimated moments at {tau.tolist()}: {est['moment'][tau].numpy()}  exact {exact[tau]}")
    assert est["count"][tau].tolist() == [4] * 5 and int(est["count"].sum()) == 20
    assert torch.isnan(est["moment"]).sum() == T - 5 and est["prediction"] == "eps"
    vf.set_moments(est)
    got = {fv: drivers.bits_per_dim(vf, data, seed=2, sample_steps=5, clip_denoised=False, fixed_variance=fv)
           for fv in ("small", "large", "analytic")}
    vf.set_moments(None)
    tot = {fv: float(r["vb"][1:].double().sum()) for fv, r in got.items()}
    print(f"sum_k>=1 vb: {tot}; analytic / small {tot['analytic'] / tot['small']:.3f}, analytic / large "
          f"{tot['analytic'] / tot['large']:.3f}")
    assert all(np.isfinite(v) for v in tot.values())
    assert torch.equal(got["small"]["x0_mse"], got["analytic"]["x0_mse"])        # the mean is untouched
    assert tot["analytic"] < 0.9 * min(tot["small"], tot["large"])


def test_rowwise_network_gives_the_same_bits_in_every_batch(gaussian):
    """Through a network whose rows do not see one another the seeded moments of a sample are the same bits whatever batch
    it stands in and wherever: what differs between batches is then the draws and this feature's kernels alone."""
    vf = gaussian["vf"]
    a = lambda rows: (gaussian["cond"][rows], [1] * len(rows), gaussian["angle"][rows], gaussian["target"][rows])  # noqa: E731
    ids = [21, 2 ** 40 + 1, 5, 8]
    whole = vf.eps_moments(*a([0, 1, 2, 3]), seed=9, sample_ids=ids)["m2"]
    assert torch.equal(whole, vf.eps_moments(*a([0, 1, 2, 3]), seed=9, sample_ids=ids)["m2"])
    back = vf.eps_moments(*a([3, 1, 0, 2]), seed=9, sample_ids=[ids[i] for i in (3, 1, 0, 2)])["m2"]
    assert torch.equal(back, whole[[3, 1, 0, 2]])
    for i in range(4):
        alone = vf.eps_moments(*a([i]), seed=9, sample_ids=[ids[i]])["m2"]
        assert torch.equal(alone[0], whole[i]), i


# ---- 5. the drivers, the checkpoint, the refusals ---------------------------------------------------------------------------------------
def test_estimate_moments_and_the_checkpoint(dev, vf, batch, tmp_path):
    from view_fusion_amd import drivers
    g = batch["gpu"]
    whole = [dict(target=g["y_0"], cond=g["y_cond"], angle=g["angle"], view_count=VC, ids=torch.tensor([7, 3]))]
    parts = [dict(target=g["y_0"][i:i + 1], cond=g["y_cond"][i:i + 1], angle=g["angle"][i:i + 1], view_count=VC[i:i + 1],
                  ids=torch.tensor([[7, 3][i]])) for i in (1, 0)]
    a = drivers.estimate_moments(vf, whole, seed=5)
    b = drivers.estimate_moments(vf, parts, seed=5)
    assert a["moment"].dtype == torch.float64 and a["moment"].shape == (T,) and not a["moment"].is_cuda
    assert a["count"].dtype == torch.int64 and a["count"].tolist() == [2] * T == b["count"].tolist()
    m2 = vf.eps_moments(g["y_cond"], VC, g["angle"], g["y_0"], seed=5, sample_ids=[7, 3])["m2"]
    assert torch.equal(a["moment"], m2.double().mean(dim=0).cpu())     # the float64 mean of the per-sample moments
    _, rec = _wiring(vf, batch, dev, None)
    tol = 4.0 * max(r[2] for r in rec)
    e = _rel(b["moment"].numpy(), a["moment"].numpy())
    print(f"estimate_moments: one batch of 2 against two of 1, reversed: rel {e:.2e} (tolerance {tol:.2e})")
    assert e <= tol
    some = drivers.estimate_moments(vf, whole + whole, seed=5, levels=[2, 9, T - 1])
    assert some["count"].nonzero().reshape(-1).tolist() == [2, 9, T - 1] and int(some["count"][9]) == 4
    assert torch.isnan(some["moment"]).sum() == T - 3
    # moments of three levels serve a chain over those levels and no other
    vf.set_moments(some)
    kw = dict(seed=1, variance="analytic", eta=1.0)
    assert torch.isfinite(_gen(vf, batch, sample_steps=[2, 9, T - 1], **kw)[4]).all()
    with pytest.raises(ValueError, match="estimated"):
        _gen(vf, batch, sample_steps=5, **kw)
    # the checkpoint carries them; state_dict() does not
    opt = torch.optim.Adam(vf.parameters(), lr=1e-4)
    path = str(tmp_path / "ck.pt")
    drivers.save_checkpoint(path, vf, opt, moments=a)
    vf.set_moments(None)
    extra = drivers.load_checkpoint(path, vf)
    vf.set_moments(extra["moments"])
    assert torch.equal(vf.moments, a["moment"]) and "moments" not in "".join(vf.state_dict())
    res = vf.bound_terms(g["y_cond"], VC, g["angle"], g["y_0"], seed=6, fixed_variance="analytic")
    small = vf.bound_terms(g["y_cond"], VC, g["angle"], g["y_0"], seed=6)
    assert torch.isfinite(res["total_bpd"]).all() and torch.equal(res["x0_mse"], small["x0_mse"])
    assert torch.equal(res["prior_bpd"], small["prior_bpd"]) and not torch.equal(res["vb"][:, 1:], small["vb"][:, 1:])
    # the drivers that forward sampler options
    first = g["y_0"]
    r = drivers.autoregressive_rollout(vf, first, steps=2, sample_steps=3, eta=1.0, seed=4, variance="analytic")
    assert r.shape == (B, 2, 3, *HW) and torch.isfinite(r).all()
    assert not torch.equal(r, drivers.autoregressive_rollout(vf, first, steps=2, sample_steps=3, eta=1.0, seed=4))
    ev = drivers.evaluate(vf, [dict(whole[0], view_count=torch.tensor(VC))], seed=3, sample_steps=3, eta=1.0,
                          variance="analytic", use_graph=False)
    assert torch.isfinite(ev["psnr"])
    vf.set_moments(None)


def test_every_refusal_comes_before_any_launch(dev, vf, batch):
    from view_fusion_amd import _lib, drivers
    g = batch["gpu"]
    gen = (g["y_cond"], VC, g["angle"])
    sc = _model(dev)
    sc.set_self_cond(0.5)
    nine = _model(dev, dict(TINY, out_channel=9))
    nine.set_learned_variance()
    nine.set_moments(np.full(T, 0.5))
    zero = _model(dev, TINY, dict(SCHED, zero_terminal_snr=True), prediction="v")
    zero.set_moments(np.full(T, 0.5))
    vf.set_moments(None)
    n0 = _lib.N_CALLS
    for kw in (dict(guidance=2.0), dict(threshold=0.9), dict(guidance=2.0, guidance_rescale=0.5), dict(levels=T + 1),
               dict(levels=[3, 5]), dict(noise=g["noise"][:, :3].contiguous())):
        with pytest.raises(ValueError):
            vf.eps_moments(*gen, g["y_0"], **kw)
    with pytest.raises(ValueError, match="self-conditioned"):
        sc.eps_moments(*gen, g["y_0"])
    with pytest.raises(ValueError, match="GPU"):
        vf.eps_moments(g["y_cond"].cpu(), VC, g["angle"].cpu(), g["y_0"].cpu())
    data = [dict(target=g["y_0"], cond=g["y_cond"], angle=g["angle"], view_count=VC)]
    with pytest.raises(ValueError, match="self-conditioned"):
        drivers.estimate_moments(sc, data)
    for call in (lambda: _gen(vf, batch, variance="analytic", sample_steps=5, eta=1.0),
                 lambda: vf.bound_terms(*gen, g["y_0"], fixed_variance="analytic"),
                 lambda: drivers.bits_per_dim(vf, data, fixed_variance="analytic")):
        with pytest.raises(ValueError, match="moments"):
            call()
    for call in (lambda: nine.generate(*gen, variance="analytic", sample_steps=5, eta=1.0),
                 lambda: nine.bound_terms(*gen, g["y_0"], fixed_variance="analytic")):
        with pytest.raises(ValueError, match="learned variance"):
            call()
    for call in (lambda: zero.generate(*gen, variance="analytic", sample_steps=5, eta=1.0),
                 lambda: zero.bound_terms(*gen, g["y_0"], fixed_variance="analytic")):
        with pytest.raises(ValueError, match="gamma = 0"):
            call()
    vf.set_moments(np.full(T, 0.5))
    with pytest.raises(ValueError, match="ddim"):
        _gen(vf, batch, variance="analytic", sample_steps=5, solver="dpmpp2m")
    with pytest.raises(ValueError, match="unknown variance"):
        _gen(vf, batch, variance="optimal", sample_steps=5)
    with pytest.raises(ValueError, match="GPU"):
        vf.bound_terms(g["y_cond"].cpu(), VC, g["angle"].cpu(), g["y_0"].cpu(), fixed_variance="analytic")
    assert _lib.N_CALLS == n0
    # guided / thresholded sampling with the analytic row is not refused: only a table row differs
    out = _gen(vf, batch, variance="analytic", sample_steps=3, eta=1.0, seed=2, guidance=1.5, threshold=0.9)
    assert torch.isfinite(out[4]).all()
    vf.set_moments(None)
