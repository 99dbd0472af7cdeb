"""CPU-only checks around the LPIPS metric: the two restatements the GPU tests rest on (tests/lpips_ref.py) against
each other and against a hand-computed toy, the state-dict mapping of drivers.LPIPS, and the host side of ops.lpips /
drivers.evaluate(lpips=)."""
import os

import numpy as np
import pytest
import torch

import lpips_ref
from conftest import ROOT


@pytest.mark.parametrize("kind", lpips_ref.KINDS)
def test_restatements_agree(kind):
    """|fp32 - fp64| is `bound`'s own e by construction; what is asserted is that e is an fp32-rounding-sized number
    (1e-4 relative, the engine's forward tolerance, is two orders above fp32 accumulation error at these depths)."""
    X, Y, net, r64, e, bnd = lpips_ref.case(kind, 2, 32, 32)
    r32 = lpips_ref.lpips_fp32(X, Y, net)
    assert r32.dtype == torch.float32 and r32.shape == (2,) and r64.dtype == np.float64 and r64.shape == (2,)
    print(f"32x32 {kind}: lpips {r64[0]:.6f} {r64[1]:.6f}  e {e:.3e}  bound {bnd.max():.3e}")
    assert float(np.abs(r32.double().numpy() - r64).max()) == e
    assert e <= 1e-4 * float(np.abs(r64).max()) + 1e-6
    assert (bnd >= 1e-6).all() and (bnd >= 4 * e).all()
    if kind != "identical":
        assert (r64 > 1e-4).all()               # 100 x the bound's floor: the parity cases are not vacuous


def test_identical_pairs_give_exactly_zero():
    X, Y, net, r64, e, _ = lpips_ref.case("identical", 2, 32, 32)
    assert (r64 == 0.0).all() and e == 0.0
    assert (lpips_ref.lpips_fp32(X, Y, net) == 0.0).all()


def test_dead_tail_network_puts_a_whole_tap_on_the_epsilon():
    X, Y, net, r64, e, _ = lpips_ref.case("noisy", 2, 32, 32, dead_tail=True)
    taps = lpips_ref._taps_fp64(X.double().numpy(), net[0])
    assert (taps[4] == 0.0).all() and (taps[3] != 0.0).any()
    assert np.isfinite(r64).all() and (r64 > 0).all()
    assert torch.isfinite(lpips_ref.lpips_fp32(X, Y, net)).all()


def test_two_tap_toy_pins_the_formula():
    """Tap 0: two channels on a 1 x 2 map.  Pixel 0: a = (3, 4) -> (0.6, 0.8), b = (0, 0) stays 0 (0 / (0 + eps)),
    d = 0.5 * 0.36 + 0.25 * 0.64 = 0.34; pixel 1: a == b, d = 0; mean over pixels 0.17.
    Tap 1: one channel, one pixel, a = 1e-10 = eps: a^ = eps / (eps + eps) = 0.5, b = 0, w = 1: d = 0.25.
    Sum over taps 0.42, less the O(eps / 5) the epsilon takes off a^ at pixel 0.  Without the epsilon tap 1 would give
    1; a sum over pixels would give 0.59."""
    a0 = np.array([[[[3.0, 1.0]], [[4.0, 2.0]]]])
    b0 = np.array([[[[0.0, 1.0]], [[0.0, 2.0]]]])
    a1, b1 = np.full((1, 1, 1, 1), 1e-10), np.zeros((1, 1, 1, 1))
    w0, w1 = np.array([0.5, 0.25]), np.array([1.0])
    got = lpips_ref.distance_fp64([a0, a1], [b0, b1], [w0, w1])
    assert got.shape == (1,) and abs(got[0] - 0.42) <= 1e-10
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    got32 = lpips_ref.distance_fp32([t(a0), t(a1)], [t(b0), t(b1)], [t(w0).reshape(1, 2, 1, 1), t(w1).reshape(1, 1, 1, 1)])
    assert got32.shape == (1,) and abs(float(got32[0]) - 0.42) <= 1e-6


def test_only_tap_terms_add_up():
    X, Y, net, r64, _, _ = lpips_ref.case("noisy", 2, 32, 32)
    parts = [lpips_ref.lpips_fp64(X, Y, lpips_ref.only_tap(net, l)) for l in range(5)]
    assert all((p > 0).all() for p in parts)
    assert np.abs(sum(parts) - r64).max() <= 1e-12


# ---- drivers.LPIPS: the state-dict mapping ---------------------------------------------------------------------------
def _prefixed(vgg, style):
    if style == "features":
        return dict(vgg)
    if style == "bare":
        return {k[len("features."):]: v for k, v in vgg.items()}
    slices = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}
    return {f"net.slice{slices[int(k.split('.')[1])]}.{k[len('features.'):]}": v for k, v in vgg.items()}


@pytest.mark.parametrize("style", ["features", "bare", "slices"])
def test_from_state_dicts_maps_every_key(style):
    from view_fusion_amd import drivers
    vgg, lin = lpips_ref.net_cached(0)
    src = _prefixed(vgg, style)
    src["classifier.0.weight"] = torch.zeros(4, 4)            # a full vgg16 state dict has more in it
    net = drivers.LPIPS.from_state_dicts(src, lin)
    assert len(net.convs) == 13 and len(net.lins) == 5
    for conv, idx in zip(net.convs, lpips_ref.CONV_IDX):
        assert torch.equal(conv.weight, vgg[f"features.{idx}.weight"]) and torch.equal(conv.bias, vgg[f"features.{idx}.bias"])
    for l, w in enumerate(net.lins):
        assert torch.equal(w, lin[f"lin{l}.model.1.weight"])
    assert all(not p.requires_grad for p in net.parameters())
    again = drivers.LPIPS()
    again.load_state_dict(net.state_dict())                    # its own state dict round-trips
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), net.state_dict().values()))
    assert all(not p.requires_grad for p in again.parameters())


def test_from_state_dicts_names_the_wrong_key():
    from view_fusion_amd import drivers
    vgg, lin = lpips_ref.net_cached(0)
    short = {k: v for k, v in vgg.items() if k != "features.17.bias"}
    with pytest.raises(KeyError, match=r"features\.17\.bias"):
        drivers.LPIPS.from_state_dicts(short, lin)
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        drivers.LPIPS.from_state_dicts(vgg, {k: v for k, v in lin.items() if not k.startswith("lin3")})
    bad = dict(vgg)
    bad["features.10.weight"] = torch.zeros(256, 64, 3, 3)
    with pytest.raises(ValueError, match=r"features\.10\.weight.*256, 64, 3, 3.*256, 128, 3, 3"):
        drivers.LPIPS.from_state_dicts(bad, lin)
    bad = _prefixed(vgg, "slices")
    bad["net.slice2.7.bias"] = torch.zeros(64)
    with pytest.raises(ValueError, match=r"net\.slice2\.7\.bias"):
        drivers.LPIPS.from_state_dicts(bad, lin)
    bad_lin = dict(lin)
    bad_lin["lin1.model.1.weight"] = torch.zeros(128)
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight"):
        drivers.LPIPS.from_state_dicts(vgg, bad_lin)


def test_from_files_reads_two_weight_files(tmp_path):
    from view_fusion_amd import drivers
    vgg, lin = lpips_ref.net_cached(0)
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    net = drivers.LPIPS.from_files(str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth"))
    assert torch.equal(net.convs[12].weight, vgg["features.28.weight"]) and torch.equal(net.lins[4], lin["lin4.model.1.weight"])


# ---- ops.lpips / evaluate: the host side -------------------------------------------------------------------------------
def test_ops_lpips_refuses_bad_shapes_before_the_library_and_cpu_tensors(monkeypatch):
    from view_fusion_amd import _lib, drivers, ops
    net = drivers.LPIPS()

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)
    for shape in [(2, 3, 16, 64), (2, 3, 64, 16), (2, 3, 40, 64), (2, 3, 64, 72), (2, 1, 64, 64)]:
        with pytest.raises(ValueError, match=str(shape)[1:-1]):
            ops.lpips(torch.rand(*shape), torch.rand(*shape), net)
    with pytest.raises(ValueError, match="2, 3, 32, 32.*2, 3, 32, 48"):
        ops.lpips(torch.rand(2, 3, 32, 32), torch.rand(2, 3, 32, 48), net)
    with pytest.raises(ValueError):
        ops.lpips(torch.rand(3, 32, 32), torch.rand(3, 32, 32), net)
    with pytest.raises(_lib.VFHipError):                      # no CPU fallback
        ops.lpips(torch.rand(2, 3, 32, 32), torch.rand(2, 3, 32, 32), net)
    with pytest.raises(_lib.VFHipError):
        net(torch.rand(2, 3, 32, 32), torch.rand(2, 3, 32, 32))
    with pytest.raises(_lib.VFHipError):
        drivers.compute_lpips(torch.rand(2, 3, 32, 32), torch.rand(2, 3, 32, 32), net)


class _Fixed(torch.nn.Module):
    """A model whose `generate` returns a fixed function of the conditioning views (as tests/test_ssim_host.py)."""

    def forward(self, y_cond, view_count, angle, generate=False):
        return (None, None, None, None, (y_cond[:, 0] * 0.75 + 0.1).contiguous())


def _eval_batches():
    g = torch.Generator().manual_seed(3)
    return [dict(target=torch.rand(B, 3, 32, 32, generator=g), cond=torch.rand(B, 6, 3, 32, 32, generator=g),
                 angle=torch.zeros(B, 1)) for B in (2, 1)]


def _host_psnr(a, b):
    return 20 * torch.log10(1.0 / torch.sqrt(torch.mean((a - b) ** 2, dim=(1, 2, 3))))


def test_evaluate_with_lpips_reports_it_through_the_same_reduction(monkeypatch):
    from view_fusion_amd import drivers
    ref = lpips_ref.net_cached(0)
    net = drivers.LPIPS.from_state_dicts(*ref)
    seen = []

    def host_lpips(a, b, n):
        seen.append(n)
        return lpips_ref.lpips_fp32(a, b, ref)
    monkeypatch.setattr(drivers, "compute_psnr", _host_psnr)
    monkeypatch.setattr(drivers, "compute_lpips", host_lpips)          # looked up at call time
    batches = _eval_batches()
    out = drivers.evaluate(_Fixed(), batches, lpips=net)
    assert set(out) == {"psnr", "lpips"} and seen and all(n is net for n in seen)
    gen = [_Fixed()(b["cond"], None, b["angle"], generate=True)[-1] for b in batches]
    want = torch.cat([lpips_ref.lpips_fp32(a, b["target"], ref) for a, b in zip(gen, batches)]).mean()
    assert out["lpips"].dim() == 0 and torch.equal(out["lpips"], want)


def test_evaluate_default_keys_are_unchanged(monkeypatch):
    from view_fusion_amd import drivers
    monkeypatch.setattr(drivers, "compute_psnr", _host_psnr)
    monkeypatch.setattr(drivers, "compute_ssim", lambda a, b: _host_psnr(a, b) * 0)
    monkeypatch.setattr(drivers, "compute_lpips", lambda *a: pytest.fail("compute_lpips called without lpips="))
    assert set(drivers.evaluate(_Fixed(), _eval_batches())) == {"psnr"}
    assert set(drivers.evaluate(_Fixed(), _eval_batches(), lpips=None, ssim=True)) == {"psnr", "ssim"}


def test_c_abi_declares_the_lpips_entry_points():
    from view_fusion_amd import _lib
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    for name in ("vf_lpips_prep", "vf_relu", "vf_relu_maxpool2", "vf_lpips_layer", "vf_lpips_layer_tiles",
                 "vf_lpips_finish", "vf_lpips_workspace_floats"):
        assert name in _lib.SIGNATURES and (name + "(") in header, name
    assert _lib._RESTYPE.get("vf_lpips_workspace_floats") is _lib._L       # a size, not an error code


def test_product_does_not_import_tests_or_oracle():
    from view_fusion_amd import drivers, ops
    assert callable(ops.lpips) and callable(drivers.compute_lpips)
    for base, _, files in os.walk(os.path.join(ROOT, "view_fusion_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(base, f)).read()
                for word in ("lpips_ref", "ssim_ref", "import oracle", "from oracle", "from tests", "import tests"):
                    assert word not in src, (f, word)
