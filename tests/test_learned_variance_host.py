"""A learned variance on the host (the head of csrc/diffusion.hip holds the definition, csrc/vlb.h the arithmetic): the
variance tables against the schedule buffers and a direct float64 formula, the library's host mirror of the KL term and
its derivative against the restatement of tests/vlb_ref.py, that restatement's closed-form gradient against float64
autograd with the residual detached, the new entry points' declarations, and every refusal that needs no device --
raised before anything touches the library.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import vlb_ref
from conftest import ROOT, TINY

SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
T = SCHED["num_timesteps"]
NINE = dict(TINY, out_channel=9)
NEW = ("vf_compose_loss_lv_fwd", "vf_compose_loss_lv_bwd", "vf_sampler_step_lv", "vf_sampler_step_lv_rng",
       "vf_sampler_step_lv_cfg", "vf_sampler_step_lv_cfg_rng", "vf_vlb_terms_host")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from view_fusion_amd import _lib
    return _lib.load()


def _cpu_model(cfg=NINE):
    from view_fusion_amd import UNet, ViewFusion
    vf = ViewFusion(UNet(**cfg), {"train": dict(SCHED)}, True, True)
    vf.set_new_noise_schedule(device=torch.device("cpu"), phase="train")
    return vf


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) < 1e-6 * np.abs(b) + 1e-7))


# ---- tables --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", [SCHED, dict(schedule="cosine", num_timesteps=50),
                                   dict(schedule="linear", num_timesteps=1000, linear_start=1e-6, linear_end=1e-2)])
def test_tables_on_the_full_schedule_are_the_buffers(sched):
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**sched)
    hi, lo = schedule.variance_tables(betas)
    bufs = schedule.schedule_tensors(betas, "cpu")
    assert hi.dtype == np.float64 and lo.dtype == np.float64
    assert np.array_equal(lo.astype(np.float32), bufs["posterior_log_variance_clipped"].numpy())      # value for value
    assert np.array_equal(hi, np.log(np.asarray(betas, dtype=np.float64)))
    assert lo[0] == np.log(1e-20) and (hi >= lo).all()
    # the explicit full chain is the same table
    h2, l2 = schedule.variance_tables(betas, np.arange(len(betas)))
    assert np.array_equal(h2, hi) and np.array_equal(l2, lo)


@pytest.mark.parametrize("K", [1, 2, 5, 7, 19])
def test_tables_on_a_strided_chain(K):
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**SCHED)
    tau = schedule.sample_timesteps(T, K)
    hi, lo = schedule.variance_tables(betas, tau)
    want_hi, want_lo = vlb_ref.tables(betas, tau)
    assert np.allclose(hi, want_hi, rtol=1e-13, atol=0) and np.allclose(lo, want_lo, rtol=1e-13, atol=0)
    assert (hi >= lo).all() and lo[0] == np.log(1e-20) and hi.shape == lo.shape == (K,)
    # exp(hi) is the chain's own beta; exp(lo) the variance sigma^2 of the ddim, eta = 1 tables
    sig = schedule.sampler_tables(betas, tau, "ddim", 1.0)["sigma"]
    assert np.allclose(np.exp(lo[1:]), sig[1:] ** 2, rtol=1e-12) and sig[0] == 0


# ---- the host mirror of csrc/vlb.h ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", ["eps", "v", "x0"])
def test_host_mirror_of_the_kl_term(lib, prediction):
    """Tolerance: the float32 evaluation of the restatement on the same inputs measures its own distance from float64;
    the mirror may be 4 x as far (expf against numpy's exp, and the header's fixed operation order), floored at the
    loss-options tolerance 1e-6 |b| + 1e-7.  Per timestep: exp(-lp) amplifies the rounding of lp at small t."""
    from view_fusion_amd import ops, schedule
    betas = schedule.make_beta_schedule(**SCHED)
    hi, lo = (x.astype(np.float32) for x in schedule.variance_tables(betas))
    c1 = schedule.schedule_tensors(betas, "cpu")["posterior_mean_coef1"].numpy()
    g32 = schedule.schedule_tensors(betas, "cpu")["gammas"].numpy()
    rng = np.random.default_rng(5)
    n = 4096
    for t in (1, 7, T - 1):
        o = rng.uniform(-1.2, 1.2, n).astype(np.float32)
        r = (rng.choice([-1.0, 1.0], n) * (0.01 + np.abs(rng.standard_normal(n)))).astype(np.float32)
        level = np.full(n, g32[t], dtype=np.float32)
        full = lambda x: np.full(n, x, dtype=np.float32)                 # noqa: E731
        lp, kl, dkl = (x.numpy() for x in ops.vlb_terms_host(o, full(hi[t]), full(lo[t]), full(c1[t]), level, r, prediction))
        ref = {}
        for dt in (np.float64, np.float32):
            m2 = dt(c1[t]) * dt(c1[t]) * vlb_ref.kappa2(prediction, level, dt) * r.astype(dt) * r.astype(dt)
            lp_r = vlb_ref.logvar(o.astype(dt), dt(hi[t]), dt(lo[t]))
            ref[dt] = (lp_r, vlb_ref.kl_bits(lp_r, dt(lo[t]), m2), vlb_ref.dkl_bits(lp_r, dt(lo[t]), m2))
            assert all(x.dtype == dt for x in ref[dt])
        for name, got, w64, w32 in zip(("lp", "kl", "dkl"), (lp, kl, dkl), ref[np.float64], ref[np.float32]):
            scale = float(np.abs(w64).max())
            e32 = float(np.abs(w32.astype(np.float64) - w64).max()) / scale
            e = float(np.abs(got.astype(np.float64) - w64).max()) / scale
            print(f"{prediction} t {t} {name}: max|.| {scale:.4g}  host mirror rel {e:.2e}  fp32 restatement rel {e32:.2e}")
            assert e <= max(4.0 * e32, 1e-6 + 1e-7 / scale), (prediction, t, name, e, e32)
    assert lib.vf_vlb_terms_host(None, None, None, None, None, None, 3, None, None, None, 0) != 0       # pred outside 0..2
    with pytest.raises(ValueError):
        ops.vlb_terms_host([0.0], [0.0, 1.0], [0.0], [0.0], [0.5], [0.0])


@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("prediction,penalty", [("eps", "mse"), ("v", "huber"), ("x0", "l1")])
def test_closed_form_gradient_is_the_detached_autograd(prediction, penalty, weighting):
    """vlb_ref.hybrid's closed-form gradient against float64 autograd of vlb_ref.hybrid_torch with r.detach(); letting the
    mean flow gives another gradient on channels 0..2."""
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**SCHED)
    hi, lo = (x.astype(np.float32) for x in schedule.variance_tables(betas))
    c1 = schedule.schedule_tensors(betas, "cpu")["posterior_mean_coef1"].numpy()
    g = torch.Generator().manual_seed(2)
    vc, H, W = [1, 3, 2], 4, 8
    out = torch.randn(sum(vc), 9, H, W, generator=g).numpy()
    out[:, 6:9] = torch.rand(sum(vc), 3, H, W, generator=g).numpy() * 2.4 - 1.2
    noise, y_0 = (torch.randn(3, 3, H, W, generator=g).numpy() for _ in range(2))
    level, t = np.array([0.99, 0.6, 0.1], dtype=np.float32), [1, 7, T - 1]
    args = (noise, y_0, vc, weighting, level, t, c1, hi, lo, 0.3, prediction, penalty, 0.7, "min_snr", 5.0, 0.0)
    ref = vlb_ref.hybrid(out, *args, gloss=1.7)
    grads = {}
    for detach in (True, False):
        o = torch.tensor(out, dtype=torch.float64, requires_grad=True)
        loss, s, vlb = vlb_ref.hybrid_torch(o, *args, detach=detach)
        (loss * 1.7).backward()
        grads[detach] = o.grad.numpy()
        if detach:
            assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * abs(ref["loss"])
            assert np.allclose(s.detach().numpy(), ref["sample_loss"], rtol=1e-12)
            assert np.allclose(vlb.detach().numpy(), ref["sample_vlb"], rtol=1e-12)
    scale = np.abs(grads[True]).max()
    assert np.abs(grads[True] - ref["dout"]).max() <= 1e-12 * scale
    assert np.abs(grads[False][:, 0:3] - grads[True][:, 0:3]).max() > 1e-3 * np.abs(grads[True][:, 0:3]).max()
    assert np.array_equal(grads[False][:, 6:9], grads[True][:, 6:9])
    if not weighting:
        assert np.all(ref["dout"][:, 3:6] == 0)


# ---- declarations ---------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_typed(lib):
    from view_fusion_amd import _lib
    from view_fusion_amd.ops import core
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/vf_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
        assert hasattr(lib, name)
        if not name.endswith("_host"):
            assert core._CALL_KIND[name] == "diffusion"
    spec = open(os.path.join(ROOT, "view_fusion_amd", "csrc", "vlb.h")).read()
    assert "vf_vlb_logvar" in spec and "vf_vlb_kl" in spec and "vf_vlb_dkl" in spec and "vf_vlb_kappa2" in spec


# ---- the setting, loss_key, the checkpoint extra ---------------------------------------------------------------------------
def test_setting_is_a_plain_attribute_and_part_of_the_loss_key():
    vf = _cpu_model()
    keys = set(vf.state_dict())
    k0 = vf.loss_key()
    assert vf.learned_variance is None and vf.last_sample_vlb is None
    vf.set_learned_variance()
    assert vf.learned_variance == 1e-3 and vf.loss_key() != k0
    k1 = vf.loss_key()
    vf.set_learned_variance(0.5)
    assert vf.learned_variance == 0.5 and vf.loss_key() not in (k0, k1)
    vf.set_learned_variance(None)
    assert vf.learned_variance is None and vf.loss_key() == k0
    assert set(vf.state_dict()) == keys and not [n for n, _ in vf.named_buffers() if "var" in n and "posterior" not in n]
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="vlb weight"):
            vf.set_learned_variance(bad)
    # the head convolution of such a network is inner_channel -> 9
    assert vf._out_channels(vf.denoise_fn) == 9 and _cpu_model(TINY)._out_channels(_cpu_model(TINY).denoise_fn) == 6


def test_checkpoint_records_the_setting(tmp_path):
    from view_fusion_amd import drivers
    vf = _cpu_model()
    opt = torch.optim.Adam(vf.parameters(), lr=1e-4)
    vf.set_learned_variance(2e-3)
    path = os.path.join(tmp_path, "lv.pt")
    drivers.save_checkpoint(path, vf, opt, it=3, learned_variance=vf.learned_variance)
    other = _cpu_model()
    for w in (None, 1e-3):
        other.set_learned_variance(w)
        with pytest.raises(ValueError, match="learned variance"):
            drivers.load_checkpoint(path, other)
    other.set_learned_variance(2e-3)
    extra = drivers.load_checkpoint(path, other)
    assert extra["learned_variance"] == 2e-3 and extra["it"] == 3
    drivers.save_checkpoint(path, vf, opt, it=4)                       # a file without the entry loads as before
    assert drivers.load_checkpoint(path, other)["it"] == 4


# ---- refusals that need no device -------------------------------------------------------------------------------------------
def test_refusals_between_the_options():
    vf, teacher = _cpu_model(), _cpu_model()
    vf.set_learned_variance()
    with pytest.raises(ValueError, match="learned variance"):
        vf.set_self_cond(0.5)
    with pytest.raises(ValueError, match="learned variance"):
        vf.set_level_sampler("fixed", bins=4, probs=[1, 1, 1, 1])
    with pytest.raises(ValueError, match="learned-variance"):
        vf.set_distill(teacher, steps=2)
    plain = _cpu_model()
    teacher.set_learned_variance()
    with pytest.raises(ValueError, match="learned-variance"):
        plain.set_distill(teacher, steps=2)                            # ... or WITH such a model
    # the other order: the setter refuses where one of the three is already on
    for prepare, word in ((lambda m: m.set_self_cond(0.5), "self-conditioning"),
                          (lambda m: m.set_level_sampler("fixed", bins=4, probs=[1, 1, 1, 1]), "level sampler"),
                          (lambda m: m.set_distill(_cpu_model(), steps=2), "distillation")):
        m = _cpu_model()
        prepare(m)
        with pytest.raises(ValueError, match=word):
            m.set_learned_variance()
        assert m.learned_variance is None


def test_refusals_when_it_runs_on_the_cpu_or_on_six_channels():
    B, H = 2, TINY["image_size"]
    args = (torch.rand(B, 2, 3, H, H), torch.tensor([2, 2]), torch.rand(B, 1))
    y = torch.rand(B, 3, H, H)
    vf = _cpu_model()
    vf.set_learned_variance()
    with pytest.raises(ValueError, match="GPU only"):
        vf(*args, y_0=y)
    with pytest.raises(ValueError, match="GPU only"):
        vf.generate(*args, sample_steps=2)
    with pytest.raises(ValueError, match="GPU only"):
        vf.p_sample(y, *args, torch.tensor([3, 3]))
    six = _cpu_model(TINY)
    six.set_learned_variance()
    for call in (lambda: six(*args, y_0=y), lambda: six.generate(*args), lambda: six.p_mean_variance(y, *args, torch.tensor([3, 3]), True)):
        with pytest.raises(ValueError, match="out_channel = 6"):
            call()
    for kw in (dict(threshold=0.9), dict(guidance=2.0, guidance_rescale=0.5)):
        with pytest.raises(ValueError, match="not built"):
            vf.generate(*args, **kw)
        with pytest.raises(ValueError, match="not built"):
            vf.p_sample(y, *args, torch.tensor([3, 3]), **kw)


def test_op_argument_errors():
    from view_fusion_amd import ops
    out6, out9 = torch.zeros(2, 6, 4, 4), torch.zeros(2, 9, 4, 4)
    off = torch.tensor([0, 1, 2], dtype=torch.int32)
    tg, lv, tab = torch.zeros(2, 3, 4, 4), torch.full((2,), 0.5), torch.zeros(T)
    t = torch.tensor([1, 2])
    with pytest.raises(ValueError, match="9 channels.*got 6 instead of 9"):
        ops.compose_loss(out6, tg, off, 2, True, lv, vlb=(t, tab, tab, tab, 1e-3))
    with pytest.raises(ValueError, match=r"\(t, c1, hi, lo, weight\)"):
        ops.compose_loss(out9, tg, off, 2, True, lv, vlb=(t, tab, tab))
    with pytest.raises(ValueError, match="vlb weight"):
        ops.compose_loss(out9, tg, off, 2, True, lv, vlb=(t, tab, tab, tab, -1.0))
    with pytest.raises(ValueError, match="one length"):
        ops.compose_loss(out9, tg, off, 2, True, lv, vlb=(t, tab, tab[:3], tab, 1e-3))
    with pytest.raises(ValueError, match="sample_scale"):
        ops.compose_loss(out9, tg, off, 2, True, lv, sample_scale=lv, vlb=(t, tab, tab, tab, 1e-3))
    tabs = {n: torch.zeros(5) for n in ("a", "b", "cy", "c0", "c1", "sigma")}
    y, k = torch.zeros(2, 3, 4, 4), torch.tensor([1, 1])
    with pytest.raises(ValueError, match="not built"):
        ops.sampler_step(out9, off, y, None, k, tabs, 2, 1, True, threshold=0.9, variance=(tab[:5], tab[:5]))
    with pytest.raises(ValueError, match=r"\(hi, lo\)"):
        ops.sampler_step(out9, off, y, None, k, tabs, 2, 1, True, variance=(tab[:5],))
    with pytest.raises(ValueError, match="variance="):
        ops.sampler_step(out9, off, y, None, k, tabs, 2, 1, True, want_logvar=True)
