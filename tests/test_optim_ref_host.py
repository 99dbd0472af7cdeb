"""CPU checks of tests/optim_ref.py (the restatement the GPU tests of the EMA / clipping extras compare with) and of the
host side of those extras: the float64 restatement against torch itself, the EMA recurrence and its warm-up against
the closed form, FusedAdam's decay schedule and argument checks, the C ABI declarations."""
import os
import re

import numpy as np
import pytest
import torch

import optim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 3, 1023, 1024, 1025, 5000)
STEPS = 5


def _inputs(seed=0):
    rng = np.random.default_rng(seed)
    params = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in SIZES]
    grads = [[((0.5 + s) * 0.01 * rng.standard_normal(n)).astype(np.float32) for n in SIZES] for s in range(STEPS)]
    return params, grads


@pytest.mark.parametrize("clip", ["active", "inactive"])
def test_f64_restatement_matches_torch_clip_and_adam(clip):
    params, grads = _inputs()
    norms = optim_ref.run_f64(params, grads)["norm"]
    max_norm = 0.5 * min(norms) if clip == "active" else 2.0 * max(norms)
    ref = optim_ref.run_f64(params, grads, lr=1e-3, max_norm=max_norm)
    assert all(s < 1.0 for s in ref["scale"]) if clip == "active" else all(s == 1.0 for s in ref["scale"])
    ps = [torch.nn.Parameter(torch.from_numpy(a).double()) for a in params]
    opt = torch.optim.Adam(ps, lr=1e-3)
    for s in range(STEPS):
        for p, g in zip(ps, grads[s]):
            p.grad = torch.from_numpy(g).double()
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        assert abs(float(total) - ref["norm"][s]) <= 1e-12 * ref["norm"][s]
        opt.step()
    for i, p in enumerate(ps):
        st = opt.state[p]
        assert optim_ref.rel_err(p.detach().numpy(), ref["p"][i]) <= 1e-12
        assert optim_ref.rel_err(st["exp_avg"].numpy(), ref["m"][i]) <= 1e-12
        assert optim_ref.rel_err(st["exp_avg_sq"].numpy(), ref["v"][i]) <= 1e-12


@pytest.mark.parametrize("warmup", [False, True])
def test_ema_recurrence_matches_the_closed_form(warmup):
    params, grads = _inputs(1)
    ref = optim_ref.run_f64(params, grads, ema_decay=0.9, ema_warmup=warmup)
    want = [min(0.9, (1.0 + t) / (10.0 + t)) if warmup else 0.9 for t in range(STEPS)]
    assert ref["decay"] == want and (not warmup or want[0] == 0.1)
    for i, p0 in enumerate(params):
        # ema_T = (prod_t d_t) ema_0 + sum_t (1 - d_t) (prod_{s > t} d_s) p_t, with ema_0 = p_0
        closed = float(np.prod(want)) * p0.astype(np.float64)
        for t in range(STEPS):
            closed = closed + (1.0 - want[t]) * float(np.prod(want[t + 1:])) * ref["p_hist"][t][i]
        assert optim_ref.rel_err(ref["ema"][i], closed) <= 1e-13


def test_f32_restatement_stays_close_to_f64():
    params, grads = _inputs(2)
    kw = dict(max_norm=0.5 * min(optim_ref.run_f64(params, grads)["norm"]), ema_decay=0.99, ema_warmup=True)
    a, b = optim_ref.run_f64(params, grads, **kw), optim_ref.run_f32(params, grads, **kw)
    # (a sanity bound, not the GPU tests' tolerance: the float 1 - float(0.999) the kernels use is 1.3e-5 off 0.001, which
    # exp_avg_sq inherits; everything else is within a few float ulps)
    for k, tol in (("p", 1e-6), ("m", 1e-6), ("v", 1e-4), ("ema", 1e-6)):
        for x, y in zip(b[k], a[k]):
            assert x.dtype == np.float32 and optim_ref.rel_err(x, y) < tol, k
    assert max(abs(x - y) / y for x, y in zip(b["norm"], a["norm"])) < 1e-6


def test_fused_adam_decay_schedule_and_argument_checks():
    from view_fusion_amd.optim import FusedAdam
    p = [torch.nn.Parameter(torch.zeros(3))]
    opt = FusedAdam(p, ema_decay=0.999, ema_warmup=True)
    for t in (0, 1, 7, 100, 100000):
        opt._ema_t = t
        d, omd = opt._ema_scalars()
        assert d == optim_ref.ema_decay_at(t, 0.999, True) == min(0.999, (1.0 + t) / (10.0 + t)) and omd == 1.0 - d
    assert FusedAdam(p, ema_decay=0.5)._ema_scalars() == (0.5, 0.5)
    plain = FusedAdam(p)
    assert not plain._extras and plain.grad_norm is None and plain.ema_decay is None and plain.max_grad_norm is None
    assert set(plain.state_dict()) == {"state", "param_groups"}
    assert set(plain.state_dict()["param_groups"][0]) == {"lr", "betas", "eps", "params"}
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(max_grad_norm=0.0), dict(ema_warmup=True)):
        with pytest.raises(ValueError):
            FusedAdam(p, **bad)
    from view_fusion_amd._lib import VFHipError
    with pytest.raises(VFHipError):
        FusedAdam(p, max_grad_norm=1.0).external_begin()
    with pytest.raises(VFHipError):
        FusedAdam(p, ema_decay=0.9).external_begin()


def test_trainer_refuses_the_extras_with_the_xgmi_reducer(monkeypatch):
    from conftest import TINY
    from view_fusion_amd import UNet, ViewFusion, train
    vf = ViewFusion(UNet(**TINY), {"train": dict(schedule="linear", num_timesteps=10, linear_start=1e-4, linear_end=0.09)})
    monkeypatch.setenv("VF_REDUCER", "xgmi")
    for kw in (dict(ema_decay=0.99), dict(max_grad_norm=1.0)):
        with pytest.raises(ValueError, match="xgmi"):
            train.Trainer(vf, **kw)


NEW = ("vf_grad_sumsq_multi", "vf_grad_norm_finish", "vf_adam_multi_ex", "vf_adam_multi_ex_dev", "vf_adam_set_scalars_ex",
       "vf_swap_multi")


def test_new_entry_points_are_declared_bound_and_mapped():
    from view_fusion_amd import _lib
    from view_fusion_amd.ops import core
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, f"{name} is not declared in include/vf_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
        assert core._CALL_KIND[name] == "adam"
    # the entry points the default path calls keep their signatures
    assert _lib.SIGNATURES["vf_adam_multi"] == [_lib._P, _lib._I, _lib._L] + [_lib._F] * 6 + [_lib._P]
    assert _lib.SIGNATURES["vf_adam_multi_dev"] == [_lib._P, _lib._I, _lib._L, _lib._P, _lib._F, _lib._F, _lib._F, _lib._P]
    assert _lib.SIGNATURES["vf_adam_set_scalars"] == [_lib._P, _lib._F, _lib._F, _lib._F, _lib._P]
