"""The analytic variance on the host (the head of csrc/diffusion.hip holds the definition): schedule.analytic_sigma2
against the Gaussian closed form and the joint Gaussian itself, the clip and the edge rows, the sampler and the bound
rows, schedule.eps_tables' algebra, the library's host mirror of one element (the function the kernel runs) against the
float32 run of tests/analytic_ref.py bit for bit, schedule.optimal_trajectory against brute-force enumeration, the new
entry points' declarations, and the refusals that need no device.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import analytic_ref
from conftest import ROOT, TINY

T50 = dict(schedule="linear", num_timesteps=50, linear_start=1e-4, linear_end=0.1)
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
PREDS = ("eps", "v", "x0")
NEW = ("vf_eps_moments", "vf_eps_moment_host")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from view_fusion_amd import _lib
    return _lib.load()


def _betas(sched):
    from view_fusion_amd import schedule
    return schedule.make_beta_schedule(**sched)


def _chains(T):
    from view_fusion_amd import schedule
    return [np.arange(T), schedule.sample_timesteps(T, 7), np.array([0, 3, 4, 17, 30, T - 1])]


# ---- the optimal variance ----------------------------------------------------------------------------------------------------
def test_sigma2_is_the_gaussian_closed_form():
    """For N(0, s^2) data the noise estimate is known exactly, and so are its moment and the variance of
    q(y_tau[k-1] | y_tau[k]): 1e-9 relative in float64, on T = 50 linear 1e-4 ... 0.1."""
    from view_fusion_amd import schedule
    betas = _betas(T50)
    worst = worst_exact = 0.0
    for tau in _chains(50):
        for eta in (0.0, 0.5, 1.0):
            for s2 in (0.25, 1.0, 3.0):
                M = analytic_ref.gaussian_moment(betas, s2)
                got = schedule.analytic_sigma2(betas, tau, M, eta)
                want = analytic_ref.gaussian_sigma2(betas, tau, eta, s2)
                assert got.dtype == np.float64 and got.shape == tau.shape
                worst = max(worst, float(np.abs(got / want - 1.0).max()))
                assert np.allclose(got, analytic_ref.sigma2(betas, tau, M, eta), rtol=1e-9, atol=0)
                if eta == 1.0:
                    exact = analytic_ref.gaussian_posterior_variance(betas, tau, s2)
                    worst_exact = max(worst_exact, float(np.abs(got / exact - 1.0).max()))
    print(f"analytic_sigma2 vs the Gaussian closed form: rel {worst:.2e}; vs the joint Gaussian at eta = 1: {worst_exact:.2e}")
    assert worst < 1e-9 and worst_exact < 1e-9


def test_moment_one_clip_and_refusals():
    from view_fusion_amd import schedule
    betas = _betas(T50)
    for tau in _chains(50):
        for eta in (0.0, 0.5, 1.0):
            lam2 = schedule.sampler_tables(betas, tau, "ddim", eta)["sigma"] ** 2
            assert np.array_equal(schedule.analytic_sigma2(betas, tau, np.ones(50), eta), lam2)      # M = 1: exactly
            zero = schedule.analytic_sigma2(betas, tau, np.zeros(50), eta)
            assert np.array_equal(schedule.analytic_sigma2(betas, tau, np.full(50, -0.3), eta), zero)  # M < 0 clipped
            assert np.array_equal(schedule.analytic_sigma2(betas, tau, np.full(50, 1.7), eta), lam2)   # M > 1 clipped
            mid = schedule.analytic_sigma2(betas, tau, np.full(50, 0.4), eta)
            assert (lam2 <= mid).all() and (mid <= zero).all() and (zero > lam2).all()                # Theorem 2
            # the sampler row: its square root with row 0 at 0, alone among the rows of the "ddim" tables
            plain = schedule.sampler_tables(betas, tau, "ddim", eta, "v")
            row = schedule.sampler_tables(betas, tau, "ddim", eta, "v", moments=np.full(50, 0.4))
            assert row["sigma"][0] == 0.0 and np.array_equal(row["sigma"][1:], np.sqrt(mid)[1:])
            assert all(np.array_equal(row[k], plain[k]) for k in plain if k != "sigma")
            one = schedule.sampler_tables(betas, tau, "ddim", eta, "v", moments=np.ones(50))["sigma"]
            assert np.array_equal(one.astype(np.float32), plain["sigma"].astype(np.float32))
    tau = _chains(50)[1]
    M = np.full(50, 0.5)
    M[int(tau[2])] = np.nan
    with pytest.raises(ValueError, match="estimated"):
        schedule.analytic_sigma2(betas, tau, M)
    M[int(tau[2])] = 0.5
    M[int(tau[2]) - 1] = np.nan                                     # a level the chain does not use
    assert np.isfinite(schedule.analytic_sigma2(betas, tau, M)).all()
    with pytest.raises(ValueError):
        schedule.analytic_sigma2(betas, tau, np.ones(49))
    with pytest.raises(ValueError, match="ddim"):
        schedule.sampler_tables(betas, tau, "dpmpp2m", 0.0, "eps", moments=np.ones(50))
    zero_snr = _betas(dict(T50, zero_terminal_snr=True))
    with pytest.raises(ValueError, match="gamma = 0"):
        schedule.analytic_sigma2(zero_snr, tau, np.ones(50))
    with pytest.raises(ValueError, match="gamma = 0"):
        schedule.nll_tables(zero_snr, tau, "v", "analytic", moments=np.ones(50))


@pytest.mark.parametrize("prediction", PREDS)
def test_bound_rows(prediction):
    from view_fusion_amd import schedule
    betas = _betas(SCHED)
    T = len(betas)
    rng = np.random.default_rng(3)
    for tau in (None, schedule.sample_timesteps(T, 5), np.array([2, 3, 11, T - 1])):
        small = schedule.nll_tables(betas, tau, prediction)
        chain = np.arange(T) if tau is None else tau
        for M in (rng.uniform(0.05, 0.95, T), np.ones(T), np.zeros(T)):
            tab = schedule.nll_tables(betas, tau, prediction, "analytic", moments=M)
            assert all(np.array_equal(tab[k], small[k]) for k in ("a", "b", "c0", "lo"))
            assert (tab["hi"] >= tab["lo"]).all()
            # rows k >= 1: log sigma*^2 at eta = 1, lambda^2 the posterior variance, by two routes
            want = analytic_ref.sigma2(betas, chain, M, 1.0)
            assert np.allclose(np.exp(tab["hi"][1:]), want[1:], rtol=1e-9, atol=0)
            assert np.allclose(tab["hi"][1:], np.log(schedule.analytic_sigma2(betas, chain, M, 1.0)[1:]), rtol=0, atol=1e-9)
            # row 0, the decoder's: never below the row "small" uses
            assert tab["hi"][0] >= small["lo"][0]
            assert np.isclose(tab["hi"][0], np.log(max(want[0], np.exp(small["lo"][0]))), rtol=1e-12, atol=0)
        floor = schedule.nll_tables(betas, tau, prediction, "analytic", moments=np.ones(T))
        assert floor["hi"][0] == small["lo"][0]                       # sigma*^2[0] = 0 at M = 1: the floor holds
        assert np.allclose(floor["hi"][1:], small["lo"][1:], rtol=0, atol=1e-12)
    for kw in (dict(fixed_variance="analytic"), dict(fixed_variance="small", moments=np.ones(T)),
               dict(fixed_variance="medium")):
        with pytest.raises(ValueError):
            schedule.nll_tables(betas, None, prediction, **kw)
    assert schedule.FIXED_VARIANCES == ("small", "large") and schedule.BOUND_VARIANCES == ("small", "large", "analytic")


# ---- the noise estimate ------------------------------------------------------------------------------------------------------
def test_eps_tables_algebra():
    """eps_hat = ea y + eb out recovers the noise that made y, for the output each prediction stands for (float64)."""
    from view_fusion_amd import schedule
    betas = _betas(SCHED)
    T = len(betas)
    gam = np.cumprod(1.0 - betas)
    rng = np.random.default_rng(0)
    x0, n = rng.uniform(-1, 1, (T, 64)), rng.standard_normal((T, 64))
    y = np.sqrt(gam)[:, None] * x0 + np.sqrt(1.0 - gam)[:, None] * n
    outs = {"eps": n, "v": np.sqrt(gam)[:, None] * n - np.sqrt(1.0 - gam)[:, None] * x0, "x0": x0}
    for prediction in PREDS:
        for tau in (None, schedule.sample_timesteps(T, 6)):
            tab = schedule.eps_tables(betas, tau, prediction)
            idx = np.arange(T) if tau is None else tau
            assert tab["ea"].dtype == np.float64 and tab["ea"].shape == idx.shape == tab["eb"].shape
            got = tab["ea"][:, None] * y[idx] + tab["eb"][:, None] * outs[prediction][idx]
            assert np.abs(got - n[idx]).max() < 1e-11, prediction
            ea, eb = analytic_ref.eps_coeffs(gam[idx], prediction)
            assert np.array_equal(ea, tab["ea"]) and np.array_equal(eb, tab["eb"])
    tab = schedule.eps_tables(betas, None, "eps")
    assert not tab["ea"].any() and (tab["eb"] == 1).all()
    with pytest.raises(ValueError):
        schedule.eps_tables(betas, None, "score")


def test_host_mirror_is_the_float32_restatement_bit_for_bit(lib):
    from view_fusion_amd import ops, schedule
    betas = _betas(SCHED)
    rng = np.random.default_rng(5)
    n = 4096
    for prediction in PREDS:
        tab = schedule.eps_tables(betas, None, prediction)
        k = rng.integers(0, len(betas), n)
        ea, eb = tab["ea"][k].astype(np.float32), tab["eb"][k].astype(np.float32)
        out = (2.0 * rng.standard_normal(n)).astype(np.float32)
        y = (1.5 * rng.standard_normal(n)).astype(np.float32)
        out[:4], y[:4] = [0.0, -0.0, 1e-3, 3e8], [1.0, 0.0, -1e-3, 1e8]
        eps, sq = ops.eps_moment_host(out, y, ea, eb)
        w_eps, w_sq = analytic_ref.eps_element(ea, eb, out, y, np.float32)
        assert w_eps.dtype == np.float32 and w_sq.dtype == np.float32
        assert np.array_equal(eps.numpy(), w_eps) and np.array_equal(sq.numpy(), w_sq)
        if prediction == "eps":                                      # eps: the output itself, to the bit
            assert np.array_equal(eps.numpy(), out)
        # against float64: two rounded products and one rounded sum, each within 2^-24 relative
        e64, _ = analytic_ref.eps_element(ea, eb, out, y)
        scale = np.abs(ea.astype(np.float64) * y) + np.abs(eb.astype(np.float64) * out)
        assert (np.abs(eps.numpy() - e64) <= 2.01 * 2.0 ** -24 * scale).all()
    with pytest.raises(ValueError):
        ops.eps_moment_host(out, y[:5], ea, eb)


# ---- the optimal trajectory --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 4, 5])
def test_optimal_trajectory_against_brute_force(K):
    from view_fusion_amd import schedule
    betas = _betas(dict(schedule="linear", num_timesteps=12, linear_start=1e-4, linear_end=0.3))
    for seed in range(4):
        M = np.random.default_rng(seed).uniform(0.05, 0.95, 12)
        for first in (0, 2):
            tau = schedule.optimal_trajectory(betas, M, K, first=first)
            want, cost = analytic_ref.brute_force_trajectory(betas, M, K, first)
            assert tau.dtype == np.int64 and tau.tolist() == list(want), (seed, first, tau, want)
            assert tau[0] == first and tau[-1] == 11 and (np.diff(tau) > 0).all()
            assert np.array_equal(schedule.sample_timesteps(12, tau), tau)            # what sample_steps= accepts
            assert np.isclose(analytic_ref.chain_cost(betas, M, tau), cost, rtol=1e-12)
            # the cost is the sum the bound's rows carry: sum_{k >= 1} hi[k] - lo[k]
            tab = schedule.nll_tables(betas, tau, "eps", "analytic", moments=M)
            assert np.isclose((tab["hi"] - tab["lo"])[1:].sum(), cost, rtol=1e-9)
            # ... and no more than that of the evenly strided chain from the same first level
            even = np.unique(np.round(np.linspace(first, 11, K)).astype(np.int64))
            assert len(even) == K and cost <= analytic_ref.chain_cost(betas, M, even) + 1e-12


def test_optimal_trajectory_edges():
    from view_fusion_amd import schedule
    betas = _betas(dict(schedule="linear", num_timesteps=12, linear_start=1e-4, linear_end=0.3))
    M = np.random.default_rng(9).uniform(0.05, 0.95, 12)
    assert schedule.optimal_trajectory(betas, M, 12).tolist() == list(range(12))
    assert schedule.optimal_trajectory(betas, M, 1, first=11).tolist() == [11]
    part = M.copy()
    part[:3] = np.nan                                                # not needed below `first`
    assert schedule.optimal_trajectory(betas, part, 3, first=3)[0] == 3
    for kw in (dict(K=1), dict(K=13), dict(K=0), dict(K=3, first=10), dict(K=2, first=11), dict(K=2.0), dict(K=3, first=-1)):
        with pytest.raises(ValueError):
            schedule.optimal_trajectory(betas, M, **kw)
    with pytest.raises(ValueError, match="estimated"):
        schedule.optimal_trajectory(betas, part, 3)
    with pytest.raises(ValueError, match="gamma = 0"):
        schedule.optimal_trajectory(_betas(dict(schedule="linear", num_timesteps=12, zero_terminal_snr=True)), M, 3)


# ---- the entry points ----------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_defined_and_typed(lib):
    from view_fusion_amd import _lib
    from view_fusion_amd.ops import core
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    source = open(os.path.join(ROOT, "view_fusion_amd", "csrc", "diffusion.hip")).read()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/vf_hip.h"
        d = re.search(r"\bint\s+" + name + r"\s*\(([^{]*?)\)\s*\{", source, re.S)
        assert d, f"{name} is not defined in csrc/diffusion.hip"
        assert len(m.group(1).split(",")) == len(d.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
        assert hasattr(lib, name)
        if not name.endswith("_host"):
            assert core._CALL_KIND[name] == "diffusion"
    assert "Analytic variance" in source and "eps_moment_kernel" in source
    # argument checks that need no device: B <= 0 returns 0 first, then null pointers / HW % 4
    assert lib.vf_eps_moments(*([None] * 8), 0, 6, 16, 4, 1, None) == 0
    assert lib.vf_eps_moments(*([None] * 8), 2, 6, 16, 4, 1, None) != 0
    assert lib.vf_eps_moment_host(*([None] * 6), 0) == 0 and lib.vf_eps_moment_host(*([None] * 6), 3) != 0
    assert lib.vf_eps_moment_host(*([None] * 6), -1) != 0


# ---- the model's attribute and the refusals that need no device --------------------------------------------------------------
def _cpu_model(cfg=TINY, sched=SCHED):
    from view_fusion_amd import UNet, ViewFusion
    vf = ViewFusion(UNet(**cfg), {"train": dict(sched)}, True, True)
    vf.set_new_noise_schedule(device=torch.device("cpu"), phase="train")
    return vf


def test_moments_are_a_plain_attribute():
    vf = _cpu_model()
    keys = list(vf.state_dict())
    assert vf.moments is None
    vf.set_moments(np.linspace(0.1, 0.9, 20))
    assert vf.moments.dtype == torch.float64 and vf.moments.shape == (20,) and not vf.moments.is_cuda
    assert list(vf.state_dict()) == keys and not any("moment" in n for n, _ in vf.named_buffers())
    vf.set_moments(dict(moment=torch.ones(20), count=torch.ones(20), prediction="eps"))   # estimate_moments' result
    assert torch.equal(vf.moments, torch.ones(20, dtype=torch.float64))
    with pytest.raises(ValueError):
        vf.set_moments(np.ones(19))
    vf.set_moments(None)
    assert vf.moments is None


def test_refusals_before_anything_touches_the_library():
    from view_fusion_amd import _lib, drivers
    vf = _cpu_model()
    y_cond, angle, y_0 = torch.rand(2, 2, 3, 16, 16), torch.rand(2, 1), torch.rand(2, 3, 16, 16)
    gen = (y_cond, [2, 2], angle)
    n0 = _lib.N_CALLS
    # estimation: guidance / threshold / rescale, a self-conditioned model, a CPU model
    for kw in (dict(guidance=2.0), dict(threshold=0.9), dict(guidance_rescale=0.5)):
        with pytest.raises(ValueError, match="guidance"):
            vf.eps_moments(y_cond, [2, 2], angle, y_0, **kw)
    with pytest.raises(ValueError, match="GPU"):
        vf.eps_moments(y_cond, [2, 2], angle, y_0)
    with pytest.raises(ValueError, match="GPU"):
        drivers.estimate_moments(vf, [dict(target=y_0, cond=y_cond, angle=angle)])
    vf.set_self_cond(0.5)
    with pytest.raises(ValueError, match="self-conditioned"):
        vf.eps_moments(y_cond, [2, 2], angle, y_0)
    vf.set_self_cond(None)
    # sampling and the bound: no moments set, dpmpp2m, an unknown name, a CPU model, a learned variance
    for call in (lambda: vf.generate(*gen, variance="analytic", sample_steps=5, eta=1.0),
                 lambda: vf(*gen, generate=True, variance="analytic"),
                 lambda: vf.p_sample(y_0, *gen, torch.tensor([3, 3]), variance="analytic"),
                 lambda: vf.bound_terms(*gen, y_0, fixed_variance="analytic"),
                 lambda: drivers.bits_per_dim(vf, [dict(target=y_0, cond=y_cond, angle=angle)], fixed_variance="analytic")):
        with pytest.raises(ValueError, match="moments"):
            call()
    vf.set_moments(np.full(20, 0.5))
    with pytest.raises(ValueError, match="ddim"):
        vf.generate(*gen, variance="analytic", sample_steps=5, solver="dpmpp2m")
    with pytest.raises(ValueError, match="unknown variance"):
        vf.generate(*gen, variance="optimal", sample_steps=5)
    with pytest.raises(ValueError, match="sampling"):
        vf(*gen, y_0=y_0, variance="analytic")
    for call in (lambda: vf.generate(*gen, variance="analytic", sample_steps=5, eta=1.0),
                 lambda: vf.p_sample(y_0, *gen, torch.tensor([3, 3]), variance="analytic"),
                 lambda: vf.bound_terms(*gen, y_0, fixed_variance="analytic")):
        with pytest.raises(ValueError, match="GPU"):
            call()
    nine = _cpu_model(dict(TINY, out_channel=9))
    nine.set_learned_variance(1e-3)
    nine.set_moments(np.full(20, 0.5))
    for call in (lambda: nine.generate(*gen, variance="analytic", sample_steps=5, eta=1.0),
                 lambda: nine.bound_terms(*gen, y_0, fixed_variance="analytic")):
        with pytest.raises(ValueError, match="learned variance"):
            call()
    other = _cpu_model(sched=dict(SCHED, num_timesteps=10))
    other._moments = torch.ones(20, dtype=torch.float64)            # moments of another schedule
    with pytest.raises(ValueError, match="levels"):
        other.generate(*gen, variance="analytic", sample_steps=5)
    assert _lib.N_CALLS == n0


def test_checkpoint_carries_the_moments(tmp_path):
    from view_fusion_amd import drivers
    vf = _cpu_model()
    opt = torch.optim.Adam(vf.parameters(), lr=1e-4)
    mom = dict(moment=torch.linspace(0.2, 0.9, 20, dtype=torch.float64), count=torch.full((20,), 4),
               prediction="eps")
    mom["moment"][3] = float("nan")
    path = str(tmp_path / "ck.pt")
    drivers.save_checkpoint(path, vf, opt, it=7, moments=mom)
    extra = drivers.load_checkpoint(path, vf)
    assert extra["it"] == 7 and extra["moments"]["prediction"] == "eps"
    assert torch.equal(torch.nan_to_num(extra["moments"]["moment"], nan=-1.0), torch.nan_to_num(mom["moment"], nan=-1.0))
    assert torch.equal(extra["moments"]["count"], mom["count"])
    vf.set_moments(extra["moments"])
    assert vf.moments.dtype == torch.float64 and torch.isnan(vf.moments[3])
    # a bare tensor records the model's own prediction
    drivers.save_checkpoint(path, vf, opt, moments=torch.ones(20))
    assert drivers.load_checkpoint(path, vf)["moments"]["prediction"] == "eps"
    # another prediction, another T: refused before anything is loaded
    vf.set_prediction("v")
    with pytest.raises(ValueError, match="prediction"):
        drivers.load_checkpoint(path, vf)
    vf.set_prediction("eps")
    with pytest.raises(ValueError, match="levels"):
        drivers.load_checkpoint(path, _cpu_model(sched=dict(SCHED, num_timesteps=10)))
    # files without the entry load as before
    drivers.save_checkpoint(path, vf, opt, it=1)
    assert "moments" not in drivers.load_checkpoint(path, vf)
