"""Classifier-free guidance on the host: the seeded conditioning-dropout draw (the library's host mirror against the
restatement of tests/guidance_ref.py, its frequency and its independence of the sample's other draws), the new entry
points' declarations, the argument errors (raised before anything touches the library) and the restatement's own
reductions at g = 1 and g = 0.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import guidance_ref
import rng_ref
import sampler_ref
from conftest import ROOT, SCHED_C1, TINY

NEW = ("vf_stack_views_cfg", "vf_draw_cond_drop", "vf_p_sample_tail_cfg", "vf_p_sample_tail_cfg_rng", "vf_sampler_step_cfg",
       "vf_sampler_step_cfg_rng")
N = 100000


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from view_fusion_amd import _lib
    return _lib.load()


def host_drop(lib, seed, ids, p):
    from view_fusion_amd import ops
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    out = np.full(ids.size, 7, dtype=np.uint8)
    rc = lib.vf_cond_drop_host(seed, ctypes.c_void_p(ids.ctypes.data), ops.cond_drop_threshold(p),
                               ctypes.c_void_p(out.ctypes.data), ids.size)
    assert rc == 0
    return out


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5, 1.0])
@pytest.mark.parametrize("seed", [0, 3, 2024, 0xDEADBEEFCAFEF00D, 2 ** 64 - 1])
def test_host_mirror_equals_the_restatement(lib, seed, p):
    from view_fusion_amd import ops
    assert ops.cond_drop_threshold(p) == guidance_ref.drop_threshold(p)
    ids = np.concatenate([np.arange(N), [2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63 - 2, 2 ** 63 - 1]]).astype(np.int64)
    got = host_drop(lib, seed, ids, p)
    want = guidance_ref.cond_drop(seed, ids, p)
    assert set(np.unique(got)) <= {0, 1} and np.array_equal(got.astype(bool), want)
    if p == 1.0:
        assert got.all()                                   # thr = 2^24: every 24-bit value is below it


def test_thresholds():
    from view_fusion_amd import ops
    assert ops.cond_drop_threshold(0.0) == 0 and ops.cond_drop_threshold(1.0) == 2 ** 24
    assert ops.cond_drop_threshold(0.1) == 1677722         # the view store's 10 % draw (csrc/rng.h)
    assert ops.cond_drop_threshold(0.5) == 2 ** 23 and ops.cond_drop_threshold(2.0 ** -30) == 1


@pytest.mark.parametrize("seed,p,stated", [(2024, 0.1, 10151), (7, 0.25, 24811)])
def test_drop_frequency(lib, seed, p, stated):
    got = int(host_drop(lib, seed, np.arange(N), p).sum())
    sd = (N * p * (1 - p)) ** 0.5
    print(f"seed {seed} p {p}: {got} of {N} dropped, {(got - N * p) / sd:+.2f} sigma")
    assert abs(got - N * p) <= 4 * sd
    assert got == stated == int(guidance_ref.cond_drop(seed, np.arange(N), p).sum())


def test_the_draw_is_independent_of_the_samples_t_and_u(lib):
    ids = np.arange(N)
    mask = host_drop(lib, 2024, ids, 0.1).astype(np.float64)
    t, u = rng_ref.train_scalars(2024, ids, 1000)
    ct, cu = float(np.corrcoef(mask, t)[0, 1]), float(np.corrcoef(mask, u)[0, 1])
    print(f"correlation of the drop mask with t {ct:+.4f}, with u {cu:+.4f}")
    assert abs(ct) < 0.02 and abs(cu) < 0.02
    # the mixed mask the GPU tests train with
    assert host_drop(lib, 3, np.arange(6), 0.5).tolist() == [0, 1, 1, 0, 1, 0]


def test_new_entry_points_are_declared_bound_and_mapped():
    from view_fusion_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    for name in NEW + ("vf_cond_drop_host",):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, f"{name} is not declared in include/vf_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    for name in NEW:
        assert ops.core._CALL_KIND[name] == "diffusion"
    # each guided tail is its sibling plus one pointer; the siblings keep their signatures
    for name in ("vf_p_sample_tail", "vf_p_sample_tail_rng", "vf_sampler_step", "vf_sampler_step_rng"):
        cfg = name.replace("_rng", "") + "_cfg" + ("_rng" if name.endswith("_rng") else "")
        assert _lib.SIGNATURES[cfg] == _lib.SIGNATURES[name][:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    assert len(_lib.SIGNATURES["vf_stack_views"]) == 16 and len(_lib.SIGNATURES["vf_stack_views_cfg"]) == 18
    assert callable(ops.draw_cond_drop) and callable(ops.guidance_scales)


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from view_fusion_amd import UNet, ViewFusion, _lib, ops

    def boom(*a, **k):
        raise AssertionError("the library was called")

    vf = ViewFusion(UNet(**TINY), {"train": SCHED_C1})
    vf.set_new_noise_schedule(device=torch.device("cpu"), phase="train")
    n_state = len(vf.state_dict())
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)
    cpu = torch.device("cpu")
    for p in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            vf.set_cond_dropout(p)
        with pytest.raises(ValueError):
            ops.draw_cond_drop(1, torch.arange(3), p)
    key = vf.loss_key()
    vf.set_cond_dropout(0.25)
    assert vf.loss_key() != key and len(vf.state_dict()) == n_state          # a key of the captured step, no buffer
    vf.set_cond_dropout()
    assert vf.loss_key() == key
    bad = (-1.0, float("nan"), float("inf"), -float("inf"), torch.tensor([1.0, -0.5]), torch.tensor([1.0, float("nan")]),
           torch.tensor([1.0, 2.0, 3.0]), torch.ones(1), [1.0])
    args = (torch.rand(2, 2, 3, 16, 16), torch.tensor([2, 1]), torch.rand(2, 1))
    for g in bad:
        with pytest.raises(ValueError):
            ops.guidance_scales(cpu, 2, g)
        with pytest.raises(ValueError):
            vf.generate(*args, guidance=g)
        with pytest.raises(ValueError):
            vf(*args, generate=True, guidance=g, sample_steps=3)
        with pytest.raises(ValueError):
            vf.p_sample(torch.rand(2, 3, 16, 16), *args, torch.tensor([3, 3]), guidance=g)
    good = ops.guidance_scales(cpu, 2, torch.tensor([0.0, 7.5], dtype=torch.float64))
    assert good.dtype == torch.float32 and good.is_contiguous() and good.tolist() == [0.0, 7.5]
    assert ops.guidance_scales(cpu, 3, 3).tolist() == [3.0, 3.0, 3.0]
    # valid arguments get as far as the first op, which refuses CPU tensors (no CPU fallback)
    with pytest.raises(_lib.VFHipError):
        vf.generate(*args, guidance=3.0)


def test_the_restatement_reduces_to_the_unguided_one():
    """guidance_ref.chain at g = 1 is sampler_ref.chain to the bit; at g = 0 it is that chain on null inputs alone."""
    from oracle import unet_ref, view_fusion_ref as vfr
    from view_fusion_amd import UNet
    from view_fusion_amd.utils import deterministic_fill_
    hw, T, vc = TINY["image_size"], SCHED_C1["num_timesteps"], [1, 3, 2]
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    unet = lambda x, a, l: unet_ref.unet_forward(sd, TINY, x, a, l)
    g = torch.Generator().manual_seed(41)
    y_cond, angle = torch.rand(3, 3, 3, hw, hw, generator=g), torch.rand(3, 1, generator=g)
    y_T, z_seq = torch.randn(3, 3, hw, hw, generator=g), torch.randn(T, 3, 3, hw, hw, generator=g)
    betas = vfr.beta_schedule(**SCHED_C1)
    gammas32 = vfr.schedule_buffers(betas)["gammas"]
    with torch.no_grad():
        for solver, eta in (("ddim", 0.5), ("dpmpp2m", 0.0)):
            tau = sampler_ref.timesteps(T, 3)
            zs = z_seq if eta else None
            plain, w_plain = sampler_ref.chain(unet, vfr.compose, betas, gammas32, tau, solver, eta, y_cond, vc, angle, y_T, zs)
            one, w_one = guidance_ref.chain(unet, betas, y_cond, vc, angle, y_T, zs, 1.0, tau=tau, solver=solver, eta=eta)
            assert torch.equal(one, plain) and all(torch.equal(a, b) for a, b in zip(w_one, w_plain))
            null, _ = sampler_ref.chain(unet, vfr.compose, betas, gammas32, tau, solver, eta, torch.zeros(3, 1, 3, hw, hw),
                                        [1, 1, 1], angle, y_T, zs)
            zero, w_zero = guidance_ref.chain(unet, betas, y_cond, vc, angle, y_T, zs, 0.0, tau=tau, solver=solver, eta=eta)
            assert torch.equal(zero, null) and not torch.equal(zero, plain)
            assert w_zero[0].shape == w_plain[0].shape                     # the weights stay the conditional ones
            three, _ = guidance_ref.chain(unet, betas, y_cond, vc, angle, y_T, zs, 3.0, tau=tau, solver=solver, eta=eta)
            assert torch.isfinite(three).all() and not torch.equal(three, plain)
        # per-sample scales: each sample follows the chain of its own scale (samples do not interact)
        mixed, _ = guidance_ref.chain(unet, betas, y_cond, vc, angle, y_T, None, [0.0, 1.0, 3.0], tau=tau, solver="dpmpp2m")
        assert torch.equal(mixed[:, 0], zero[:, 0]) and torch.equal(mixed[:, 1], one[:, 1]) and torch.equal(mixed[:, 2], three[:, 2])
        # the ancestral chain at g = 1 against the fp32 oracle's own chain (fp32 against float64: the chain tolerance)
        anc, _ = guidance_ref.chain(unet, betas, y_cond, vc, angle, y_T, z_seq, 1.0)
        ref = vfr.generate(unet, vfr.schedule_buffers(betas), y_cond, vc, angle, y_T, z_seq)[0]
        assert float((anc[-1] - ref).abs().max()) <= 1e-3
