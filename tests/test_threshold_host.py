"""Dynamic thresholding and guidance rescaling on the host: the restatement of tests/threshold_ref.py against
torch.quantile / torch.std written out, the (k, frac) helper at its edges, the new entry points' declarations and the
argument errors (raised before anything touches the library).  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import threshold_ref
from conftest import ROOT, SCHED_C1, TINY

NEW = ("vf_compose_eps", "vf_sample_stat", "vf_abs_quantile", "vf_p_sample_tail_eps", "vf_p_sample_tail_eps_rng",
       "vf_sampler_step_eps", "vf_sampler_step_eps_rng")


@pytest.mark.parametrize("shape", [(3, 3, 16, 16), (2, 3, 4, 5), (1, 3, 1, 1)])
@pytest.mark.parametrize("q", [0.001, 0.5, 0.9, 0.995, 1.0])
def test_the_threshold_is_torch_quantile_with_clamp_and_divide(shape, q):
    g = torch.Generator().manual_seed(7 + shape[-1])
    y0_hat = (2.5 * torch.randn(*shape, generator=g)).double()
    y0_hat[0].mul_(0.1)                                      # one sample whose quantile is below 1: s = 1
    for c in (None, 1.5):
        s = torch.quantile(y0_hat.abs().flatten(1), q, dim=1).clamp_min(1.0)
        if c is not None:
            s = s.clamp_max(c)
        sb = s.reshape(-1, 1, 1, 1)
        want = torch.maximum(torch.minimum(y0_hat, sb), -sb) / sb
        got, s_ref = threshold_ref.bound(y0_hat.numpy(), q, c)
        # frac is rounded to float32 in the definition, torch.quantile keeps it in float64: 2^-24 of the gap
        assert np.allclose(s_ref, s.numpy(), rtol=1e-7, atol=0) and s_ref[0] == 1.0
        assert np.allclose(got, want.numpy(), rtol=1e-7, atol=1e-12) and np.abs(got).max() <= 1.0
    static, none = threshold_ref.bound(y0_hat.numpy())
    assert none is None and np.array_equal(static, y0_hat.clamp(-1, 1).numpy())
    assert np.array_equal(threshold_ref.bound(y0_hat.numpy(), clip=False)[0], y0_hat.numpy())


@pytest.mark.parametrize("phi", [0.3, 0.7, 1.0])
def test_the_rescale_is_the_formula_with_torch_std(phi):
    g = torch.Generator().manual_seed(11)
    eps_c = torch.randn(3, 3, 16, 16, generator=g).double()
    eps_g = (3.0 * eps_c - 2.0 * torch.randn(3, 3, 16, 16, generator=g).double())
    eps_g[2] = 0.25                                          # a constant sample: sigma(eps_g) == 0 -> r = 1
    r = threshold_ref.rescale_factor(eps_c.numpy(), eps_g.numpy(), phi)
    for unbiased in (False, True):                            # the same n in both: n against n - 1 cancels
        sc, sg = eps_c.flatten(1).std(dim=1, unbiased=unbiased), eps_g.flatten(1).std(dim=1, unbiased=unbiased)
        want = phi * (sc / sg) + (1 - phi)
        assert np.allclose(r[:2], want[:2].numpy(), rtol=1e-12)
    assert r[2] == 1.0 and (r[:2] < 1.0).all()
    if phi == 1.0:                                            # the rescaled noise has the conditional one's deviation
        scaled = r[:2, None] * eps_g[:2].flatten(1).numpy()
        assert np.allclose(scaled.std(axis=1), eps_c[:2].flatten(1).numpy().std(axis=1), rtol=1e-12)


def test_quantile_position_helper():
    from view_fusion_amd import ops
    assert ops.quantile_position(768, 1.0) == (767, 0.0)                 # q = 1: x[k+1] does not exist
    assert ops.quantile_position(1, 0.3) == (0, 0.0) and ops.quantile_position(1, 1.0) == (0, 0.0)     # n = 1
    assert ops.quantile_position(769, 0.5) == (384, 0.0)                 # an integer position
    assert ops.quantile_position(5, 0.25) == (1, 0.0) and ops.quantile_position(768, 0.0) == (0, 0.0)
    k, frac = ops.quantile_position(768, 0.5)
    assert k == 383 and frac == 0.5
    k, frac = ops.quantile_position(768, 0.995)
    assert k == 763 and frac == float(np.float32(0.995 * 767 - 763))
    k, frac = ops.quantile_position(768, 766 / 767)                      # k = n - 2, whatever the rounding of q (n - 1)
    assert (k, frac) in ((766, 0.0), (765, float(np.float32(766 / 767 * 767 - 765))))
    assert ops.quantile_position(3, 1.0 - 2.0 ** -40) == (2, 0.0)        # a frac that rounds to 1 in float32
    for n, q in ((60, 0.37), (2880, 0.9), (73728, 0.995), (12288, 1e-4)):
        k, frac = ops.quantile_position(n, q)
        assert (k, frac) == threshold_ref.quantile_position(n, q) and 0 <= k < n and 0.0 <= frac < 1.0
    for n, q in ((0, 0.5), (4, -0.1), (4, 1.1), (4, float("nan"))):
        with pytest.raises(ValueError):
            ops.quantile_position(n, q)


def test_new_entry_points_are_declared_bound_and_mapped():
    from view_fusion_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, f"{name} is not declared in include/vf_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
        assert ops.core._CALL_KIND[name] == "diffusion"
    assert _lib.SIGNATURES["vf_abs_quantile"] == [_lib._P, _lib._I, _lib._I, _lib._I, _lib._F, _lib._P, _lib._P]
    assert callable(ops.abs_quantile) and callable(ops.threshold_settings) and callable(ops.threshold_scratch)


BAD = [dict(threshold=0.0), dict(threshold=-0.5), dict(threshold=1.01), dict(threshold=float("nan")),
       dict(threshold=0.9, threshold_max=0.99), dict(threshold=0.9, threshold_max=float("nan")), dict(threshold_max=1.5),
       dict(guidance=3.0, guidance_rescale=-0.1), dict(guidance=3.0, guidance_rescale=1.2),
       dict(guidance=3.0, guidance_rescale=float("nan")), dict(guidance_rescale=0.7)]


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from view_fusion_amd import UNet, ViewFusion, _lib, drivers, ops

    def boom(*a, **k):
        raise AssertionError("the library was called")

    vf = ViewFusion(UNet(**TINY), {"train": SCHED_C1})
    vf.set_new_noise_schedule(device=torch.device("cpu"), phase="train")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)
    args = (torch.rand(2, 2, 3, 16, 16), torch.tensor([2, 1]), torch.rand(2, 1))
    y, t = torch.rand(2, 3, 16, 16), torch.tensor([3, 3])
    for kw in BAD:
        guided = "guidance" in kw
        with pytest.raises(ValueError):
            ops.threshold_settings(**{k: v for k, v in kw.items() if k != "guidance"}, guided=guided)
        with pytest.raises(ValueError):
            vf.generate(*args, **kw)
        with pytest.raises(ValueError):
            vf(*args, generate=True, sample_steps=3, **kw)
        with pytest.raises(ValueError):
            vf.p_sample(y, *args, t, **kw)
        with pytest.raises(ValueError):
            vf.p_mean_variance(y, *args, t, True, **kw)
        with pytest.raises(ValueError):
            drivers.evaluate(vf, [dict(target=y, cond=args[0], angle=args[2], view_count=args[1])], **kw)
        with pytest.raises(ValueError):
            drivers.autoregressive_rollout(vf, y, steps=2, **kw)
    # threshold= replaces the clamp: not without it
    with pytest.raises(ValueError):
        vf.p_sample(y, *args, t, clip_denoised=False, threshold=0.9)
    with pytest.raises(ValueError):
        vf.p_mean_variance(y, *args, t, False, threshold=0.9)
    with pytest.raises(ValueError):
        ops.threshold_settings(threshold=0.9, clip=False)
    # the tails themselves refuse before their first launch (CPU tensors: any launch would raise VFHipError instead)
    off = torch.tensor([0, 2, 3], dtype=torch.int32)
    out = torch.rand(3, 6, 16, 16)
    for kw in BAD:
        kw = {k: v for k, v in kw.items() if k != "guidance"}
        with pytest.raises(ValueError):
            ops.p_sample_tail(out, off, y, None, t, vf._sched(), 2, 2, True, **kw)
        with pytest.raises(ValueError):
            ops.sampler_step(out, off, y, None, t, {}, 2, 2, True, **kw)
    # what is accepted: the edges of the ranges; guidance_rescale = 0 is "off", with or without guidance
    assert ops.threshold_settings() == (None, float("inf"), 0.0)
    assert ops.threshold_settings(1.0, 1.0, 1.0, guided=True) == (1.0, 1.0, 1.0)
    assert ops.threshold_settings(guidance_rescale=0) == (None, float("inf"), 0.0)
    assert ops.threshold_settings(guidance_rescale=0.0, guided=True)[2] == 0.0
    assert ops.threshold_settings(0.995, guidance_rescale=0.7, guided=True) == (0.995, float("inf"), 0.7)
    # valid arguments get as far as the first op, which refuses CPU tensors (no CPU fallback)
    with pytest.raises(_lib.VFHipError):
        vf.generate(*args, guidance=3.0, threshold=0.995, guidance_rescale=0.7)
    with pytest.raises(_lib.VFHipError):
        vf.generate(*args, guidance_rescale=0)
    with pytest.raises(ValueError):
        ops.abs_quantile(torch.rand(5), 0.5)
    with pytest.raises(ValueError):
        ops.abs_quantile(torch.rand(2, 5), 1.5)
