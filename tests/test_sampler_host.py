"""Few-step sampling on the host: the timestep selection and the tables of view_fusion_amd/schedule.py against the
float64 restatement of tests/sampler_ref.py and against the ancestral sampler's own buffers, the new entry points'
declarations, and generate()'s argument errors (raised before anything touches the library).  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import sampler_ref
from conftest import ROOT, SCHED_C1, SCHED_TEST, SCHED_TRAIN, TINY
from view_fusion_amd import schedule

SCHEDS = {"c1": SCHED_C1, "test": SCHED_TEST, "train": SCHED_TRAIN}          # T = 10, 1000, 2000
CASES = [("ddim", 0.0), ("ddim", 0.5), ("ddim", 1.0), ("dpmpp2m", 0.0)]


def _betas(name):
    return schedule.make_beta_schedule(**SCHEDS[name])


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


@pytest.mark.parametrize("T", [10, 1000, 2000])
def test_sample_timesteps(T):
    for K in (1, 2, 3, 7, T):
        tau = schedule.sample_timesteps(T, K)
        assert tau.dtype == np.int64 and tau.shape == (K,)
        assert tau[-1] == T - 1 and tau[0] >= 0 and (np.diff(tau) > 0).all()
        assert np.array_equal(tau, sampler_ref.timesteps(T, K))
        # an explicit sequence (list, array or tensor) is taken as it is
        assert np.array_equal(schedule.sample_timesteps(T, tau.tolist()), tau)
        assert np.array_equal(schedule.sample_timesteps(T, torch.tensor(tau)), tau)
    assert np.array_equal(schedule.sample_timesteps(T, T), np.arange(T))
    assert np.array_equal(schedule.sample_timesteps(T, np.int64(2)), [T // 2 - 1, T - 1])
    for bad in (0, -1, T + 1, 2.0, True, [], [0, T - 2], [3, 3, T - 1], [5, 2, T - 1], [-1, T - 1], [0.5, T - 1],
                [0, T]):
        with pytest.raises(ValueError):
            schedule.sample_timesteps(T, bad)


@pytest.mark.parametrize("sched", list(SCHEDS))
def test_tables_against_the_restatement(sched):
    betas = _betas(sched)
    T = len(betas)
    for K in (1, 2, 3, 5, T):
        tau = schedule.sample_timesteps(T, K)
        for solver, eta in CASES:
            got = schedule.sampler_tables(betas, tau, solver, eta)
            want = sampler_ref.tables(betas, tau, solver, eta)
            assert set(got) == set(schedule.TABLE_NAMES)
            for name in schedule.TABLE_NAMES:
                assert got[name].dtype == np.float64 and got[name].shape == (K,)
                assert np.isfinite(got[name]).all(), (name, K)
                assert name in "ab" or np.abs(got[name]).max() <= 2.8, (name, K)      # a, b grow like 1 / sqrt(gamma)
                np.testing.assert_allclose(got[name], want[name], rtol=1e-6, atol=0, err_msg=f"{solver} {eta} {K} {name}")
            # the last step lands on y0 itself, without noise; the first executed step has no history
            assert got["cy"][0] == 0 and got["c0"][0] == 1 and got["sigma"][0] == 0 and got["c1"][0] == 0
            assert got["c1"][-1] == 0
            assert (got["sigma"] == 0).all() if eta == 0 else (got["sigma"][1:] > 0).all()
            assert (got["c1"][1:-1] != 0).all() if solver == "dpmpp2m" else not got["c1"].any()


@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_ddim_direction_coefficient_where_the_textbook_difference_cancels(eta):
    """cy sigma_t = sqrt(sigma_p^2 - s^2): at T = 1000, K = 2 the second level is e^-35 below the first and the
    difference, taken in float64, keeps no digit at eta = 1.  Both the product and the restatement avoid it; here the
    difference itself, in 60-digit decimal arithmetic from the same float64 betas."""
    from decimal import Decimal, getcontext
    getcontext().prec = 60
    betas = _betas("test")
    tau = schedule.sample_timesteps(1000, 2)
    gam = [Decimal(1)]
    for v in betas:
        gam.append(gam[-1] * (1 - Decimal(float(v))))
    gt, gp = gam[int(tau[1]) + 1], gam[int(tau[0]) + 1]
    s2 = Decimal(eta) ** 2 * (1 - gp) / (1 - gt) * (1 - gt / gp)
    want = float(((1 - gp - s2) / (1 - gt)).sqrt())
    for tab in (schedule.sampler_tables(betas, tau, "ddim", eta), sampler_ref.tables(betas, tau, "ddim", eta)):
        assert abs(tab["cy"][1] - want) <= 1e-6 * want, (tab["cy"][1], want)


@pytest.mark.parametrize("sched", list(SCHEDS))
def test_full_length_ddim_eta1_is_the_ancestral_sampler(sched):
    """K = T, eta = 1: cy / c0 round to the very fp32 posterior_mean_coef2 / posterior_mean_coef1 of the default
    sampler, a / b are its sqrt_recip(m1)_gammas, and sigma^2 is the posterior variance."""
    betas = _betas(sched)
    T = len(betas)
    tab = schedule.sampler_tables(betas, schedule.sample_timesteps(T, T), "ddim", 1.0)
    buf = {k: v.numpy() for k, v in schedule.schedule_tensors(betas, "cpu").items()}
    assert np.array_equal(_f32(tab["c0"]), buf["posterior_mean_coef1"])
    assert np.array_equal(_f32(tab["cy"]), buf["posterior_mean_coef2"])
    assert np.array_equal(_f32(tab["a"]), buf["sqrt_recip_gammas"])
    assert np.array_equal(_f32(tab["b"]), buf["sqrt_recipm1_gammas"])
    gam = np.cumprod(1.0 - betas)
    var = betas * (1.0 - np.append(1.0, gam[:-1])) / (1.0 - gam)
    assert tab["sigma"][0] == 0 and var[0] == 0
    np.testing.assert_allclose(tab["sigma"][1:] ** 2, var[1:], rtol=1e-6, atol=0)


@pytest.mark.parametrize("sched", list(SCHEDS))
def test_dpmpp2m_at_two_steps_is_ddim_eta0(sched):
    """Both of its steps are first order, and the first-order DPM-Solver++ step is the deterministic DDIM step."""
    betas = _betas(sched)
    tau = schedule.sample_timesteps(len(betas), 2)
    a, d = schedule.sampler_tables(betas, tau, "dpmpp2m", 0.0), schedule.sampler_tables(betas, tau, "ddim", 0.0)
    for name in schedule.TABLE_NAMES:
        np.testing.assert_allclose(a[name], d[name], rtol=1e-12, atol=0, err_msg=name)
        assert np.array_equal(_f32(a[name]), _f32(d[name])), name           # the device tables are the same bits


def test_sampler_argument_errors():
    betas = _betas("c1")
    tau = schedule.sample_timesteps(10, 5)
    for solver, eta in (("dpmpp2m", 0.5), ("ddim", -0.1), ("ddim", 1.5), ("euler", 0.0), (None, 0.0)):
        with pytest.raises(ValueError):
            schedule.sampler_tables(betas, tau, solver, eta)


def test_generate_rejects_bad_arguments_before_any_library_call(monkeypatch):
    from view_fusion_amd import UNet, ViewFusion, _lib

    def boom(*a, **k):
        raise AssertionError("the library was called")

    vf = ViewFusion(UNet(**TINY), {"train": SCHED_C1})
    vf.set_new_noise_schedule(device=torch.device("cpu"), phase="train")
    before = list(vf.state_dict())
    assert vf.betas64.dtype == np.float64 and "betas64" not in before and len(before) == len(UNet(**TINY).state_dict()) + 6
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)
    args = (torch.rand(2, 2, 3, 16, 16), torch.tensor([2, 1]), torch.rand(2, 1))
    for kw in (dict(sample_steps=0), dict(sample_steps=11), dict(sample_steps=[0, 5]), dict(sample_steps=5, solver="heun"),
               dict(sample_steps=5, eta=1.5), dict(sample_steps=5, eta=-0.5), dict(sample_steps=5, solver="dpmpp2m", eta=0.5)):
        with pytest.raises(ValueError):
            vf.generate(*args, **kw)
        with pytest.raises(ValueError):
            vf(*args, generate=True, **kw)
    # valid arguments get as far as the first op, which refuses CPU tensors (no CPU fallback)
    with pytest.raises(_lib.VFHipError):
        vf.generate(*args, sample_steps=5, solver="dpmpp2m")


def test_new_entry_points_are_declared_bound_and_mapped():
    from view_fusion_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    for name in ("vf_sampler_step", "vf_sampler_step_rng"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, f"{name} is not declared in include/vf_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
        assert ops.core._CALL_KIND[name] == "diffusion"
    assert callable(ops.sampler_step)
    # the default sampler's entries keep their signatures
    assert len(_lib.SIGNATURES["vf_p_sample_tail"]) == 20 and len(_lib.SIGNATURES["vf_p_sample_tail_rng"]) == 21
