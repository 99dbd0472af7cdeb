"""v- and x0-prediction on the CPU: the host mirror of the native loss weights (csrc/loss_weight.h) against float64, the
(a, b) table pairs of schedule.prediction_tables, the zero-terminal-SNR rescale and what it does to every sampler table,
argument errors, the checkpoint check, the state_dict and the C ABI.  No GPU."""
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

import loss_ref
import prediction_ref
from conftest import GOLDEN, ROOT, TINY

LEVELS = np.array([0.95, 0.4, 0.05], dtype=np.float32)
WEIGHT_CASES = [(None, 0.0, 0.0), ("min_snr", 5.0, 0.0), ("p2", 1.0, 1.0)]
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from view_fusion_amd import _lib
    return _lib.load()


def _model(sched=SCHED):
    from view_fusion_amd import UNet, ViewFusion
    vf = ViewFusion(UNet(**TINY), {"train": dict(sched)})
    vf.set_new_noise_schedule(device=torch.device("cpu"), phase="train")
    return vf


# ---- weights ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,a,b", WEIGHT_CASES)
@pytest.mark.parametrize("prediction", prediction_ref.PREDICTIONS)
def test_weight_host_mirror_against_float64(lib, prediction, kind, a, b):
    """test_loss_host's bound: |host - float64| <= 4 e, e the distance of the float32 restatement from float64."""
    from view_fusion_amd import ops
    out = ops.loss_weights_pred_host(LEVELS, prediction, kind, a, b).numpy()
    w64 = prediction_ref.weights(LEVELS, prediction, kind, a, b)
    w32 = prediction_ref.weights(LEVELS, prediction, kind, a, b, np.float32)
    assert out.dtype == np.float32 and np.isfinite(out).all() and np.isfinite(w64).all()
    e = float(np.abs(w32.astype(np.float64) - w64).max())
    err = float(np.abs(out.astype(np.float64) - w64).max())
    print(f"{prediction} {kind}({a}, {b}): w64 {w64}  float32 restatement e {e:.3e}  |host - fp64| {err:.3e}  bound {4 * e:.3e}")
    assert err <= 4.0 * e, (err, e)
    if prediction == "eps":                                    # the eps column is the existing mirror, bit for bit
        import ctypes
        old = np.empty(3, dtype=np.float32)
        code = {None: 0, "min_snr": 1, "p2": 2}[kind]
        assert lib.vf_loss_weights_host(ctypes.c_void_p(LEVELS.ctypes.data), 3, code, a, b,
                                        ctypes.c_void_p(old.ctypes.data)) == 0
        assert np.array_equal(old, out)
    if kind is None:
        assert (out == 1).all()


@pytest.mark.parametrize("kind,a,b", WEIGHT_CASES[1:])
def test_weight_identities(kind, a, b):
    """w_v = w_eps g and w_x0 = w_eps g / (1 - g): the header's closed forms in float64 against the definition."""
    g = LEVELS.astype(np.float64)
    w_eps = loss_ref.weights(LEVELS, kind, a, b)
    snr = g / (1.0 - g)
    if kind == "min_snr":
        v, x0 = np.minimum(g, a * (1.0 - g)), np.minimum(snr, a)
        assert (w_eps < 1).any() and (w_eps == 1).any()        # both sides of the min
    else:
        v, x0 = np.power(a + snr, -b) * g, np.power(a + snr, -b) * snr
    np.testing.assert_allclose(v, w_eps * g, rtol=1e-14)
    np.testing.assert_allclose(x0, w_eps * snr, rtol=1e-14)
    np.testing.assert_allclose(prediction_ref.weights(LEVELS, "v", kind, a, b), v, rtol=1e-14)
    np.testing.assert_allclose(prediction_ref.weights(LEVELS, "x0", kind, a, b), x0, rtol=1e-14)


def test_weight_host_mirror_rejects_unknown_codes(lib):
    import ctypes
    out = np.zeros(3, dtype=np.float32)
    for pred, kind in ((-1, 0), (3, 0), (1, 3), (2, -1)):
        assert lib.vf_loss_weights_pred_host(ctypes.c_void_p(LEVELS.ctypes.data), 3, pred, kind, 1.0, 1.0,
                                             ctypes.c_void_p(out.ctypes.data)) != 0


# ---- tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", prediction_ref.PREDICTIONS)
def test_tables_recover_y0(prediction):
    """a y_t - b target == y_0 in float64, 1e-12 relative, every t of a T = 20 schedule."""
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**SCHED)
    a, b = schedule.prediction_tables(betas, prediction)
    ra, rb = prediction_ref.tables(betas, prediction)
    np.testing.assert_allclose(a, ra, rtol=1e-14)
    # "eps": the product keeps the reference's sqrt(1 / g - 1), whose difference cancels near g = 1: 2^-52 / (1 - g[0])
    np.testing.assert_allclose(b, rb, rtol=4 * 2.0 ** -52 / (1.0 - np.cumprod(1.0 - betas)[0]), atol=0)
    g = np.cumprod(1.0 - betas)
    rng = np.random.default_rng(5)
    y_0, noise = rng.standard_normal((20, 3, 4, 4)), rng.standard_normal((20, 3, 4, 4))
    lv = g.reshape(-1, 1, 1, 1)
    y_t = np.sqrt(lv) * y_0 + np.sqrt(1.0 - lv) * noise
    tg = prediction_ref.target(prediction, noise, y_0, g)
    got = a.reshape(-1, 1, 1, 1) * y_t - b.reshape(-1, 1, 1, 1) * tg
    err = float(np.abs(got - y_0).max() / np.abs(y_0).max())
    print(f"{prediction}: max |a y_t - b target - y_0| / max|y_0| = {err:.2e}")
    assert err <= 1e-12
    # the few-step tables gather the same pair; cy, c0, c1, sigma do not depend on the prediction
    tau = schedule.sample_timesteps(20, 5)
    for solver, eta in (("ddim", 0.0), ("ddim", 1.0), ("dpmpp2m", 0.0)):
        eps_tab = schedule.sampler_tables(betas, tau, solver, eta)
        tab = schedule.sampler_tables(betas, tau, solver, eta, prediction)
        assert np.array_equal(tab["a"], a[tau]) and np.array_equal(tab["b"], b[tau])
        assert all(np.array_equal(tab[n], eps_tab[n]) for n in ("cy", "c0", "c1", "sigma"))


def test_eps_tables_are_the_buffers():
    """The "eps" pair rounds to the very fp32 values of the two schedule buffers."""
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**SCHED)
    a, b = schedule.prediction_tables(betas, "eps")
    bufs = schedule.schedule_tensors(betas, "cpu")
    assert torch.equal(torch.tensor(a, dtype=torch.float32), bufs["sqrt_recip_gammas"])
    assert torch.equal(torch.tensor(b, dtype=torch.float32), bufs["sqrt_recipm1_gammas"])


# ---- zero terminal SNR -----------------------------------------------------------------------------------------------
def test_zero_terminal_snr_rescale():
    from view_fusion_amd import schedule
    T = 20
    plain = schedule.make_beta_schedule(**SCHED)
    betas = schedule.make_beta_schedule(**SCHED, zero_terminal_snr=True)
    assert np.array_equal(betas, schedule.rescale_zero_terminal_snr(plain))
    assert np.array_equal(schedule.make_beta_schedule(**SCHED, zero_terminal_snr=False), plain)
    g0, g = np.cumprod(1.0 - plain), np.cumprod(1.0 - betas)
    assert g[-1] == 0.0 and g0[-1] > 0
    assert abs(g[0] - g0[0]) <= 1e-14 * g0[0]
    assert (np.diff(g) < 0).all() and betas[-1] == 1.0 and (betas > 0).all()
    # Lin et al.: sqrt(gamma) is an affine image of the old one
    r0, r = np.sqrt(g0), np.sqrt(g)
    np.testing.assert_allclose(r, (r0 - r0[-1]) * r0[0] / (r0[0] - r0[-1]), rtol=1e-12, atol=1e-15)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                        # the expected warnings are silenced inside, nothing else is
        bufs = schedule.schedule_tensors(betas, "cpu")
        for name in ("posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2"):
            assert torch.isfinite(bufs[name]).all(), name
        for prediction in ("v", "x0"):
            a, b = schedule.prediction_tables(betas, prediction)
            assert np.isfinite(a).all() and np.isfinite(b).all()
            for K in (1, 2, 3, T):
                tau = schedule.sample_timesteps(T, K)
                for solver, eta in (("ddim", 0.0), ("ddim", 1.0), ("dpmpp2m", 0.0)):
                    tab = schedule.sampler_tables(betas, tau, solver, eta, prediction)
                    for n, v in tab.items():
                        assert np.isfinite(v).all(), (prediction, K, solver, eta, n, v)
                    if solver == "dpmpp2m" and K >= 3:          # next to lambda = -inf: first order
                        assert tab["c1"][K - 2] == 0.0 and not np.signbit(tab["c1"][K - 2])
                        first = schedule.sampler_tables(betas, tau, "ddim", 0.0, prediction)
                        assert abs(tab["c0"][K - 2] - first["c0"][K - 2]) <= 1e-12
        for K in (1, 3, T):
            for solver in ("ddim", "dpmpp2m"):
                with pytest.raises(ValueError):
                    schedule.sampler_tables(betas, schedule.sample_timesteps(T, K), solver, 0.0, "eps")


def test_eps_sampling_on_a_zero_terminal_schedule_raises_before_any_launch():
    vf = _model(dict(SCHED, zero_terminal_snr=True))
    assert float(vf.gammas[-1]) == 0.0
    y = torch.zeros(1, 3, 16, 16)
    cond, angle, t = torch.zeros(1, 1, 3, 16, 16), torch.zeros(1, 1), torch.tensor([19])
    for call in (lambda: vf.generate(cond, [1], angle), lambda: vf.generate(cond, [1], angle, sample_steps=3),
                 lambda: vf.p_sample(y, cond, [1], angle, t), lambda: vf.p_mean_variance(y, cond, [1], angle, t, True),
                 lambda: vf(cond, [1], angle, generate=True)):
        with pytest.raises(ValueError, match="zero"):         # (a CPU model: a launch would raise VFHipError instead)
            call()
    vf.set_prediction("v")
    vf._check_samplable()
    for k, v in vf._sched().items():
        assert torch.isfinite(v).all(), k


# ---- the model's switch ------------------------------------------------------------------------------------------------
def test_set_prediction_is_a_plain_attribute():
    ref = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))["tiny"]
    vf = _model()
    assert vf.prediction == "eps"
    key = vf.loss_key()
    sched = vf._sched()
    assert all(sched[k] is getattr(vf, k) for k in sched)       # the very buffer tensors
    vf.set_prediction("v")
    assert vf.prediction == "v" and vf.loss_key() != key
    assert [k for k, _ in vf.state_dict().items()] == [k for k, _ in ref]
    assert len(list(vf.buffers())) == 6 and not [n for n, _ in vf.named_buffers() if "pred" in n]
    sv = vf._sched()
    assert sv["posterior_mean_coef1"] is vf.posterior_mean_coef1 and sv["sqrt_recip_gammas"] is not vf.sqrt_recip_gammas
    g = torch.tensor(np.cumprod(1.0 - vf.betas64))            # (float64: 1 - g cancels in the fp32 buffer)
    assert torch.allclose(sv["sqrt_recip_gammas"].double(), g.sqrt(), rtol=1e-6, atol=0)
    assert torch.allclose(sv["sqrt_recipm1_gammas"].double(), (1 - g).sqrt(), rtol=1e-6, atol=0)
    vf.set_prediction("x0")
    sx = vf._sched()
    assert (sx["sqrt_recip_gammas"] == 0).all() and (sx["sqrt_recipm1_gammas"] == -1).all()
    # predict_start: y0 back from y_t and the prediction's own target, for all three
    rng = torch.Generator().manual_seed(2)
    y_0, noise = torch.randn(4, 3, 8, 8, generator=rng), torch.randn(4, 3, 8, 8, generator=rng)
    t = torch.tensor([1, 7, 12, 19])
    lv = vf.gammas[t].reshape(-1, 1, 1, 1)
    y_t = vf.q_sample(y_0, lv, noise)
    for p in prediction_ref.PREDICTIONS:
        vf.set_prediction(p)
        tg = torch.tensor(prediction_ref.target(p, noise.numpy(), y_0.numpy(), lv.numpy())).float()
        assert torch.allclose(vf.predict_start(y_t, t, tg), y_0, atol=2e-5), p
    vf.set_prediction()
    assert vf.prediction == "eps" and vf.loss_key() == key
    assert torch.equal(vf.predict_start(y_t, t, noise), vf.predict_start_from_noise(y_t, t, noise))
    with pytest.raises(ValueError):
        vf.set_prediction("velocity")
    assert vf.prediction == "eps"                               # a refused call changes nothing


def test_sampler_plan_follows_the_prediction():
    vf = _model()
    tau = [4, 9, 14, 19]
    pe = vf._sampler_plan(tau, "ddim", 0.0, torch.device("cpu"))
    assert vf._sampler_plan(tau, "ddim", 0.0, torch.device("cpu")) is pe
    vf.set_prediction("v")
    pv = vf._sampler_plan(tau, "ddim", 0.0, torch.device("cpu"))
    assert pv is not pe and not torch.equal(pv["a"], pe["a"])
    assert all(torch.equal(pv[n], pe[n]) for n in ("cy", "c0", "c1", "sigma", "tau", "level"))


def test_argument_errors():
    from view_fusion_amd import ops, schedule
    out, noise = torch.zeros(1, 6, 4, 4), torch.zeros(1, 3, 4, 4)
    off, level = torch.tensor([0, 1], dtype=torch.int32), torch.tensor([0.5])
    with pytest.raises(ValueError, match="unknown prediction"):
        ops.compose_loss(out, noise, off, 1, True, level, prediction="velocity", y_0=noise)
    for p in ("v", "x0"):
        with pytest.raises(ValueError, match="y_0"):
            ops.compose_loss(out, noise, off, 1, True, level, prediction=p)
    with pytest.raises(ValueError, match="y_0"):
        ops.compose_loss(out, noise, off, 1, True, level, y_0=noise)
    with pytest.raises(ValueError):
        schedule.prediction_tables(schedule.make_beta_schedule(**SCHED), "score")
    with pytest.raises(ValueError):
        schedule.sampler_tables(schedule.make_beta_schedule(**SCHED), [9, 19], "ddim", 0.0, "score")
    with pytest.raises(ValueError):
        ops.loss_weights_pred_host(LEVELS, "score")


def test_load_checkpoint_refuses_another_prediction(tmp_path):
    from view_fusion_amd import drivers
    vf = _model()
    vf.set_prediction("v")
    opt = torch.optim.SGD(vf.parameters(), lr=0.1)
    path = str(tmp_path / "v.pt")
    drivers.save_checkpoint(path, vf, opt, it=3, prediction=vf.prediction)
    other = _model()
    before = [p.detach().clone() for p in other.parameters()]
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    with pytest.raises(ValueError, match="prediction"):
        drivers.load_checkpoint(path, other)
    assert all(torch.equal(p, q + 1.0) for p, q in zip(other.parameters(), before))       # nothing was loaded
    other.set_prediction("v")
    extras = drivers.load_checkpoint(path, other)
    assert extras["prediction"] == "v" and extras["it"] == 3
    assert all(torch.equal(p, q) for p, q in zip(other.parameters(), vf.parameters()))
    plain = str(tmp_path / "plain.pt")                                 # a file without the entry loads as before
    drivers.save_checkpoint(plain, vf, opt, it=4)
    assert drivers.load_checkpoint(plain, _model())["it"] == 4 and "prediction" not in drivers.load_checkpoint(plain, other)


def test_abi_has_the_prediction_entries(lib):
    from view_fusion_amd import _lib
    from view_fusion_amd.ops import core
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    for name, n in (("vf_compose_loss_pred_fwd", 25), ("vf_compose_loss_pred_bwd", 17), ("vf_loss_weights_pred_host", 7)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/vf_hip.h"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name]) == n, name
        assert hasattr(lib, name)
    F_, I_ = _lib._F, _lib._I
    assert _lib.SIGNATURES["vf_compose_loss_pred_fwd"][13:24] == [I_, I_, I_, I_, I_, F_, I_, F_, F_, I_, I_]
    assert _lib.SIGNATURES["vf_compose_loss_pred_bwd"][9:16] == [I_, I_, I_, I_, I_, F_, I_]
    assert _lib.SIGNATURES["vf_loss_weights_pred_host"][1:6] == [I_, I_, I_, F_, F_]
    assert core._CALL_KIND["vf_compose_loss_pred_fwd"] == core._CALL_KIND["vf_compose_loss_pred_bwd"] == "diffusion"
