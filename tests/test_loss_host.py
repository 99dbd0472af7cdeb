"""The loss options on the CPU: tests/loss_ref.py against torch autograd built the reference's way, the library's host
mirror of the weight function (csrc/loss_weight.h) against float64, ViewFusion.set_loss's argument checks and the C ABI.
No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn.utils.rnn import pad_sequence

import loss_ref
from conftest import GOLDEN, ROOT, TINY

VC = (1, 3, 2)
WEIGHT_CASES = [(None, 0.0, 0.0), ("min_snr", 5.0, 0.0), ("min_snr", 1.0, 0.0), ("p2", 1.0, 1.0), ("p2", 1.0, 0.5),
                ("p2", 0.5, 2.0)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from view_fusion_amd import _lib
    return _lib.load()


def _torch_loss(out, target, vc, weighting, w, penalty, delta):
    """pad_sequence with -inf -> softmax over the views -> the functional loss per sample -> times w -> mean."""
    per_sample = torch.split(out, list(vc))
    eps = pad_sequence([o[:, :3] for o in per_sample], batch_first=True)
    if weighting:
        logits = pad_sequence([o[:, 3:] for o in per_sample], batch_first=True, padding_value=float("-inf"))
        nh = (eps * torch.softmax(logits, dim=1)).sum(dim=1)
    else:
        nh = torch.stack([o[:, :3].mean(dim=0) for o in per_sample])
    fn = {"mse": F.mse_loss, "l1": F.l1_loss, "huber": lambda a, b: F.huber_loss(a, b, delta=delta)}[penalty]
    s = torch.stack([fn(nh[b], target[b]) for b in range(len(vc))])
    return (s * w).mean(), s


@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("kind,a,b", [(None, 0.0, 0.0), ("min_snr", 5.0, 0.0), ("p2", 1.0, 1.0)])
@pytest.mark.parametrize("penalty", loss_ref.PENALTIES)
def test_restatement_against_torch_autograd(penalty, kind, a, b, weighting):
    g = torch.Generator().manual_seed(5)
    out = torch.randn(sum(VC), 6, 8, 8, generator=g, dtype=torch.float64) * 2
    target = torch.randn(len(VC), 3, 8, 8, generator=g, dtype=torch.float64)
    level = np.array([0.95, 0.4, 0.05], dtype=np.float32)             # min_snr(5): w = 5/19, 1, 1
    delta = 0.7
    ref = loss_ref.loss(out.numpy(), target.numpy(), VC, weighting, level, penalty, delta, kind, a, b, gloss=1.7)
    w = torch.from_numpy(loss_ref.weights(level, kind, a, b))
    if kind == "min_snr":
        assert w[0] < 1 and w[1] == 1 and w[2] == 1
    if penalty == "huber":                                            # both branches are in play
        frac = float((np.abs(ref["d"]) <= delta).mean())
        assert 0.1 < frac < 0.9, frac
    ot = out.clone().requires_grad_(True)
    lt, st = _torch_loss(ot, target, VC, weighting, w, penalty, delta)
    (lt * 1.7).backward()
    assert abs(ref["loss"] - float(lt.detach())) <= 1e-13 * abs(float(lt.detach()))
    assert np.abs(ref["sample_loss"] - st.detach().numpy()).max() <= 1e-13 * float(st.detach().max())
    assert np.abs(ref["dout"] - ot.grad.numpy()).max() <= 1e-13 * float(ot.grad.abs().max())
    assert np.all(ref["dout"][0, 3:] == 0)                            # the single-view sample: zero logit gradient
    if not weighting:
        assert np.all(ref["dout"][:, 3:] == 0)


def test_binning_restatement():
    level = np.array([0.0, 0.0999999, 0.1, 0.55, 0.999999, 1.0], dtype=np.float32)
    assert loss_ref.bins(level, 10).tolist() == [0, 0, 1, 5, 9, 9]
    s, c = loss_ref.histogram(level, np.arange(6.0), 10)
    assert c.tolist() == [2, 1, 0, 0, 0, 1, 0, 0, 0, 2] and s.tolist() == [1.0, 2.0, 0, 0, 0, 3.0, 0, 0, 0, 9.0]


def _levels():
    """Levels the project's schedules produce: every gamma of every schedule of the fixture, and training draws
    (g[t] - g[t-1]) u + g[t-1] between neighbours of the two schedules the configs use."""
    z = np.load(os.path.join(GOLDEN, "schedules.npz"))
    gam = [z[k] for k in z.files if k.endswith(".gammas")]
    rng = np.random.default_rng(0)
    for k in ("linear_train.gammas", "linear_test.gammas"):
        g = z[k]
        u = rng.random(g.size - 1).astype(np.float32)
        gam.append((g[1:] - g[:-1]) * u + g[:-1])
    lv = np.concatenate(gam).astype(np.float32)
    assert lv.min() == min(g.min() for g in gam) and lv.max() == max(g.max() for g in gam)
    return lv


@pytest.mark.parametrize("kind,a,b", WEIGHT_CASES)
def test_weight_host_mirror_against_float64(lib, kind, a, b):
    lv = _levels()
    assert lv.size > 5000 and lv.min() == 0.0 and lv.max() > 0.99999
    out = np.full(lv.size, np.nan, dtype=np.float32)
    code = {None: 0, "min_snr": 1, "p2": 2}[kind]
    assert lib.vf_loss_weights_host(ctypes.c_void_p(lv.ctypes.data), lv.size, code, a, b,
                                    ctypes.c_void_p(out.ctypes.data)) == 0
    w64 = loss_ref.weights(lv, kind, a, b)
    w32 = loss_ref.weights(lv, kind, a, b, np.float32)
    assert np.isfinite(w64).all() and np.isfinite(out).all()
    e = float(np.abs(w32.astype(np.float64) - w64).max())
    err = float(np.abs(out.astype(np.float64) - w64).max())
    print(f"{kind}({a}, {b}): {lv.size} levels in [{lv.min():.3e}, {lv.max():.7f}]  w in [{w64.min():.3e}, {w64.max():.3e}]"
          f"  float32 restatement e {e:.3e}  |host - fp64| {err:.3e}  bound {4 * e:.3e}")
    assert err <= 4.0 * e, (err, e)
    if kind == "min_snr":
        assert (w64 == 1).any() and (w64 < 1).any() and out[lv == 0.0].tolist() == [1.0] * int((lv == 0.0).sum())
    if kind is None:
        assert (out == 1).all()


def test_weight_host_mirror_rejects_unknown_kinds(lib):
    lv, out = np.array([0.5], dtype=np.float32), np.zeros(1, dtype=np.float32)
    for kind in (-1, 3):
        assert lib.vf_loss_weights_host(ctypes.c_void_p(lv.ctypes.data), 1, kind, 1.0, 1.0,
                                        ctypes.c_void_p(out.ctypes.data)) != 0


def test_set_loss_validates_and_stores_no_state():
    from view_fusion_amd import UNet, ViewFusion
    vf = ViewFusion(UNet(**TINY), {"train": dict(schedule="linear", num_timesteps=10, linear_start=1e-4, linear_end=0.09)})
    keys = list(vf.state_dict().keys())
    vf.set_loss()
    assert vf._loss is None
    vf.set_loss(penalty="huber", delta=0.5, weighting="min_snr", snr_gamma=3.0)
    assert vf._loss == dict(penalty="huber", delta=0.5, weight_kind="min_snr", a=3.0, b=0.0)
    vf.set_loss(weighting="p2", p2_k=2.0, p2_gamma=0.5)
    assert vf._loss == dict(penalty="mse", delta=1.0, weight_kind="p2", a=2.0, b=0.5)
    key = vf.loss_key()
    vf.set_loss(weighting="p2", p2_k=2.0, p2_gamma=1.0)
    assert vf.loss_key() != key
    for bad in (dict(penalty="l2"), dict(weighting="snr"), dict(delta=0.0), dict(delta=-1.0), dict(snr_gamma=0.0),
                dict(snr_gamma=-5.0), dict(p2_k=-0.1), dict(penalty="huber", delta=float("nan"))):
        with pytest.raises(ValueError):
            vf.set_loss(**bad)
    assert vf._loss == dict(penalty="mse", delta=1.0, weight_kind="p2", a=2.0, b=1.0)       # a refused call changes nothing
    vf.set_loss()
    assert vf._loss is None and list(vf.state_dict().keys()) == keys
    assert not [n for n, _ in vf.named_buffers() if "loss" in n]


def test_trainer_refuses_a_histogram_without_the_gpu():
    from view_fusion_amd import UNet, ViewFusion, train
    vf = ViewFusion(UNet(**TINY), {"train": dict(schedule="linear", num_timesteps=10, linear_start=1e-4, linear_end=0.09)})
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            train.Trainer(vf, loss_bins=bad)
    with pytest.raises(ValueError):
        train.Trainer(vf, loss_bins=8)                                # a CPU model: the kernels fill the histogram
    with pytest.raises(ValueError):
        train.Trainer(vf).loss_by_level()


def test_abi_has_the_loss_entries(lib):
    from view_fusion_amd import _lib
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    for name, n in (("vf_compose_loss_fwd", 22), ("vf_compose_loss_bwd", 14), ("vf_loss_weights_host", 6)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/vf_hip.h"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name]) == n, name
        assert hasattr(lib, name)
    # the floats of the two launchers sit where the header says
    F_, I_ = _lib._F, _lib._I
    assert _lib.SIGNATURES["vf_compose_loss_fwd"][11:21] == [I_, I_, I_, I_, I_, F_, I_, F_, F_, I_]
    assert _lib.SIGNATURES["vf_compose_loss_bwd"][7:13] == [I_, I_, I_, I_, I_, F_]
    assert _lib.SIGNATURES["vf_loss_weights_host"][1:5] == [I_, I_, F_, F_]
