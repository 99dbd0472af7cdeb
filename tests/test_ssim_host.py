"""CPU-only checks around the SSIM metric: the two restatements the GPU tests rest on (tests/ssim_ref.py) against each
other and against closed forms, the C-ABI surface of vf_ssim, and the host side of ops.ssim / drivers.evaluate."""
import os
import re

import numpy as np
import pytest
import torch

import ssim_ref
from conftest import ROOT

# max |ssim_fp32 - ssim_fp64| measured per input class on this case table, times two.  The flat classes are large
# because the fp32 window does not sum to exactly 1, so E[x^2] - mu_x^2 does not cancel against C2 = 9e-4.
FP32_DEVIATION = {"rand_rand": 2 * 2.4e-7, "noisy": 2 * 8e-6, "ident": 0.0, "const": 2 * 1.19e-4,
                  "flat_noise": 2 * 4.9e-5}


@pytest.mark.parametrize("kind", ssim_ref.CLASSES)
@pytest.mark.parametrize("H,W", ssim_ref.SIZES)
def test_fp32_restatement_against_fp64(H, W, kind):
    X, Y = ssim_ref.make_pair(kind, 2, 3, H, W)
    r32, r64 = ssim_ref.ssim_fp32(X, Y), ssim_ref.ssim_fp64(X, Y)
    assert r32.dtype == torch.float32 and r64.dtype == np.float64 and r32.shape == (2,) and r64.shape == (2,)
    err = float(np.abs(r32.double().numpy() - r64).max())
    print(f"{H}x{W} {kind}: ssim {r64[0]:+.6f}  |fp32 - fp64| {err:.3e}")
    assert err <= FP32_DEVIATION[kind]


@pytest.mark.parametrize("H,W", ssim_ref.SIZES)
def test_closed_forms(H, W):
    X, Y = ssim_ref.make_pair("ident", 2, 3, H, W)
    assert (ssim_ref.ssim_fp64(X, Y) == 1.0).all() and (ssim_ref.ssim_fp32(X, Y) == 1.0).all()
    X, Y = ssim_ref.make_pair("const", 2, 3, H, W)
    a, b, C1 = 0.25, 0.75, 0.01 ** 2
    want = (2 * a * b + C1) / (a * a + b * b + C1)                   # both variances and the covariance are zero
    assert abs(want - 0.60006) < 1e-5
    assert np.abs(ssim_ref.ssim_fp64(X, Y) - want).max() <= 1e-12


@pytest.mark.parametrize("kind", ["rand_rand", "noisy", "flat_noise"])
def test_fp64_is_symmetric(kind):
    X, Y = ssim_ref.make_pair(kind, 2, 3, 24, 40)
    assert np.abs(ssim_ref.ssim_fp64(X, Y) - ssim_ref.ssim_fp64(Y, X)).max() <= 1e-14


def test_data_range_scales_out_in_fp64():
    X, Y = ssim_ref.make_pair("noisy", 2, 3, 24, 40)
    assert np.abs(ssim_ref.ssim_fp64(X.double() * 255, Y.double() * 255, 255.0) - ssim_ref.ssim_fp64(X, Y)).max() <= 1e-10


def _declared_arity(header, name):
    m = re.search(r"\b(?:int|long)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/vf_hip.h"
    return len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))


def test_c_abi_declares_ssim_with_matching_arity():
    from view_fusion_amd import _lib
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    for name in ("vf_ssim", "vf_ssim_workspace_floats"):
        assert name in _lib.SIGNATURES, name
        assert _declared_arity(header, name) == len(_lib.SIGNATURES[name]), name
    assert _lib._RESTYPE.get("vf_ssim_workspace_floats") is _lib._L       # a size, not an error code


def test_drivers_has_compute_ssim():
    from view_fusion_amd import drivers
    assert callable(drivers.compute_ssim)


class _Fixed(torch.nn.Module):
    """A model whose `generate` returns a fixed function of the conditioning views (as tests/test_ddp_gloo.py)."""

    def forward(self, y_cond, view_count, angle, generate=False):
        return (None, None, None, None, (y_cond[:, 0] * 0.75 + 0.1).contiguous())


def _eval_batches():
    g = torch.Generator().manual_seed(3)
    return [dict(target=torch.rand(B, 3, 16, 16, generator=g), cond=torch.rand(B, 6, 3, 16, 16, generator=g),
                 angle=torch.zeros(B, 1)) for B in (2, 3)]


def _host_psnr(a, b):
    return 20 * torch.log10(1.0 / torch.sqrt(torch.mean((a - b) ** 2, dim=(1, 2, 3))))


def _patch_host_metrics(monkeypatch):
    from view_fusion_amd import drivers
    monkeypatch.setattr(drivers, "compute_psnr", _host_psnr)
    monkeypatch.setattr(drivers, "compute_ssim", ssim_ref.ssim_fp32)
    return drivers


def test_evaluate_with_ssim_reports_both_metrics(monkeypatch):
    drivers = _patch_host_metrics(monkeypatch)
    batches = _eval_batches()
    out = drivers.evaluate(_Fixed(), batches, ssim=True)
    assert set(out) == {"psnr", "ssim"}
    gen = [_Fixed()(b["cond"], None, b["angle"], generate=True)[-1] for b in batches]
    for k, fn in (("psnr", _host_psnr), ("ssim", ssim_ref.ssim_fp32)):
        want = torch.cat([fn(a, b["target"]) for a, b in zip(gen, batches)]).mean()
        assert out[k].dim() == 0 and torch.equal(out[k], want), k
    more = drivers.evaluate(_Fixed(), batches, ssim=True,
                            extra_metrics={"mse": lambda a, b: ((a - b) ** 2).mean(dim=(1, 2, 3))})
    assert set(more) == {"psnr", "ssim", "mse"}


def test_evaluate_default_reports_psnr_only(monkeypatch):
    drivers = _patch_host_metrics(monkeypatch)
    monkeypatch.setattr(drivers, "compute_ssim", lambda a, b: pytest.fail("compute_ssim called without ssim=True"))
    out = drivers.evaluate(_Fixed(), _eval_batches())
    assert set(out) == {"psnr"}


def test_ops_ssim_refuses_bad_shapes_before_the_library(monkeypatch):
    from view_fusion_amd import _lib, ops

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)
    with pytest.raises(ValueError, match="10, 64"):
        ops.ssim(torch.rand(2, 3, 10, 64), torch.rand(2, 3, 10, 64))
    with pytest.raises(ValueError, match="64, 10"):
        ops.ssim(torch.rand(2, 3, 64, 10), torch.rand(2, 3, 64, 10))
    with pytest.raises(ValueError, match="2, 3, 16, 16.*2, 3, 16, 17"):
        ops.ssim(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 17))
    with pytest.raises(ValueError):
        ops.ssim(torch.rand(3, 16, 16), torch.rand(3, 16, 16))
