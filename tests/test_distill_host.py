"""Progressive distillation on the host: the grids and target weights (schedule.distill_tables) against the float64
restatement of tests/distill_ref.py, the identity "one student step on x~ = the teacher's two steps", the seeded draw of the
student step against tests/rng_ref.py, the truncated-SNR weight's host mirror, set_distill's argument errors and that the
teacher stays outside the module tree.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import distill_ref
import loss_ref
import prediction_ref
import rng_ref
from conftest import GOLDEN, SCHED_TRAIN, TINY

SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)       # the sampler tests' T = 20
SCHED_ZT = dict(SCHED, zero_terminal_snr=True)
LEVELS = np.array([0.95, 0.4, 0.05], dtype=np.float32)                                       # loss_ref's tests' levels
CASES = [(SCHED, "eps", K) for K in (1, 2, 3, 4, 5, 7, 10)] + [(SCHED_ZT, "v", K) for K in (1, 2, 3, 4, 5, 7, 10)] + \
        [(SCHED_TRAIN, "eps", K) for K in (4, 64, 1000)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from view_fusion_amd import _lib
    return _lib.load()


def _model(sched=SCHED, unet=TINY):
    from view_fusion_amd import UNet, ViewFusion
    vf = ViewFusion(UNet(**unet), {"train": dict(sched)})
    vf.set_new_noise_schedule(device=torch.device("cpu"), phase="train")
    return vf


# ---- tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched,prediction,K", CASES, ids=[f"T{s['num_timesteps']}-{p}-K{K}" for s, p, K in CASES])
def test_distill_tables(sched, prediction, K):
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**sched)
    d = schedule.distill_tables(betas, K, prediction)
    ref = distill_ref.grids(betas, K)
    assert d["tau_s"].dtype == np.int64 and np.array_equal(d["tau_t"][1::2], d["tau_s"])
    assert np.array_equal(d["tau_s"], ref["tau_s"]) and np.array_equal(d["tau_t"], ref["tau_t"])
    assert d["tau_s"][-1] == len(betas) - 1 and d["tau_t"][-1] == len(betas) - 1
    w1, w2 = d["w1"], d["w2"]
    assert w1.dtype == np.float64 and w1.shape == (K,) and (w1 >= 0).all() and (w1 <= 1).all() and w1[0] == 0
    assert np.array_equal(w2, 1.0 - w1)
    np.testing.assert_allclose(w1, ref["w1"], rtol=0, atol=1e-12)
    assert d["teacher"]["a"].shape == (2 * K,) and np.isfinite(d["teacher"]["a"]).all() and np.isfinite(d["teacher"]["b"]).all()
    assert not d["teacher"]["sigma"].any() and not d["teacher"]["c1"].any()
    # one student step on x~ == the teacher's two steps, for random z, x1, x2
    rng = np.random.default_rng(11)
    z, x1, x2 = rng.standard_normal((3, K, 64))
    t, s = d["teacher"], d["student"]
    zp = t["cy"][1::2, None] * z + t["c0"][1::2, None] * x1
    zpp = t["cy"][0::2, None] * zp + t["c0"][0::2, None] * x2
    got = s["cy"][:, None] * z + s["c0"][:, None] * (w1[:, None] * x1 + w2[:, None] * x2)
    err = float(np.abs(got - zpp).max())
    # ... and the paper's quotient form gives the same x~ where its denominator c0_S is not tiny
    quot = (zpp - s["cy"][:, None] * z) / s["c0"][:, None]
    qerr = float(np.abs(quot - (w1[:, None] * x1 + w2[:, None] * x2)).max())
    print(f"T {len(betas)} {prediction} K {K}: identity max-abs {err:.2e}  quotient form max-abs {qerr:.2e}  "
          f"min c0_S {s['c0'].min():.3e}  w1 in [{w1.min():.3f}, {w1.max():.3f}]")
    assert err <= 1e-12
    assert qerr <= 1e-12 / s["c0"].min()


def test_distill_tables_refuse_bad_step_counts():
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**SCHED)
    for K in (0, -1, 11, 20, 2.0, True):
        with pytest.raises(ValueError):
            schedule.distill_tables(betas, K)
    schedule.distill_tables(betas, 10)
    with pytest.raises(ValueError):                       # an eps teacher on a zero-terminal-SNR schedule
        schedule.distill_tables(schedule.make_beta_schedule(**SCHED_ZT), 4, "eps")


# ---- the draw of i -----------------------------------------------------------------------------------------------------
def test_step_draw_host_mirror(lib):
    from view_fusion_amd import ops
    seed = 0xD15717
    ids = np.concatenate([np.arange(4000), [2 ** 33 + 5, 2 ** 62 - 1]]).astype(np.int64)
    for K in (1, 2, 3, 4, 10, 1000):
        got = ops.distill_step_host(seed, torch.from_numpy(ids), K).numpy()
        want = distill_ref.draw_step(seed, ids, K)
        assert got.dtype == np.int64 and np.array_equal(got, want), K
        assert got.min() >= 0 and got.max() <= K - 1
        if K <= 10:
            assert set(got.tolist()) == set(range(K)), K       # every value reachable
    # a sample's i depends on (seed, id) alone: not on the batch it is in, nor on its row
    K = 7
    full = ops.distill_step_host(seed, torch.from_numpy(ids[:64]), K).numpy()
    perm = np.random.default_rng(0).permutation(64)
    assert np.array_equal(ops.distill_step_host(seed, torch.from_numpy(ids[perm]), K).numpy(), full[perm])
    assert np.array_equal(ops.distill_step_host(seed, torch.from_numpy(ids[10:13]), K).numpy(), full[10:13])
    assert not np.array_equal(ops.distill_step_host(seed + 1, torch.from_numpy(ids[:64]), K).numpy(), full)
    # the word is the one that gives t otherwise
    t, _ = rng_ref.train_scalars(seed, ids[:64], 8)
    assert np.array_equal(t - 1, full)
    out = np.zeros(2, dtype=np.int64)
    for K in (0, -3, 2 ** 27 + 1):
        assert lib.vf_distill_step_host(seed, ctypes.c_void_p(ids.ctypes.data), K, ctypes.c_void_p(out.ctypes.data), 2) != 0
    with pytest.raises(ValueError):
        ops.distill_step_host(seed, [0, 1], 0)


# ---- the truncated-SNR weight ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", prediction_ref.PREDICTIONS)
def test_trunc_snr_host_mirror_against_float64(lib, prediction):
    """test_loss_host's bound: |host - float64| <= 4 e, e the distance of the float32 restatement from float64."""
    from view_fusion_amd import ops
    out = ops.loss_weights_pred_host(LEVELS, prediction, "trunc_snr").numpy()
    w64 = distill_ref.trunc_snr(LEVELS, prediction)
    w32 = distill_ref.trunc_snr(LEVELS, prediction, np.float32)
    e = float(np.abs(w32.astype(np.float64) - w64).max())
    err = float(np.abs(out.astype(np.float64) - w64).max())
    print(f"trunc_snr {prediction}: w64 {w64}  host {out}  float32 restatement e {e:.3e}  |host - fp64| {err:.3e}")
    assert out.dtype == np.float32 and err <= 4.0 * e + 0.0
    assert np.all(np.abs(out - w64) < 1e-6 * np.abs(w64) + 1e-7)                 # close()
    g = LEVELS.astype(np.float64)
    snr = g / (1.0 - g)
    want = {"eps": np.maximum(snr, 1.0) / snr, "v": np.maximum(snr, 1.0) / snr * g, "x0": np.maximum(snr, 1.0)}[prediction]
    np.testing.assert_allclose(w64, want, rtol=1e-14)
    assert (w64 > prediction_ref.c(LEVELS, prediction)).any() and (w64 == prediction_ref.c(LEVELS, prediction)).any()


def test_other_weight_kinds_keep_their_host_values(lib):
    """The existing kinds' mirrors, bit for bit against their float32 restatement's neighbourhood, and their codes."""
    from view_fusion_amd import ops
    assert ops.diffusion.WEIGHT_KINDS == {None: 0, "none": 0, "min_snr": 1, "p2": 2, "trunc_snr": 3}
    want = {("eps", "min_snr"): loss_ref.weights(LEVELS, "min_snr", 5.0, 0.0, np.float32),
            ("v", "min_snr"): prediction_ref.weights(LEVELS, "v", "min_snr", 5.0, 0.0, np.float32),
            ("x0", "min_snr"): prediction_ref.weights(LEVELS, "x0", "min_snr", 5.0, 0.0, np.float32)}
    for (pred, kind), w in want.items():           # fminf and the fp32 arithmetic of these forms are exact operations
        assert np.array_equal(ops.loss_weights_pred_host(LEVELS, pred, kind, 5.0, 0.0).numpy(), w), (pred, kind)
    for pred in prediction_ref.PREDICTIONS:
        assert (ops.loss_weights_pred_host(LEVELS, pred, None).numpy() == 1).all()
        p2 = ops.loss_weights_pred_host(LEVELS, pred, "p2", 1.0, 1.0).numpy().astype(np.float64)
        np.testing.assert_allclose(p2, prediction_ref.weights(LEVELS, pred, "p2", 1.0, 1.0), rtol=1e-6)
    out = np.zeros(3, dtype=np.float32)
    for pred in (-1, 3):
        assert lib.vf_loss_weights_trunc_snr_host(ctypes.c_void_p(LEVELS.ctypes.data), 3, pred,
                                                  ctypes.c_void_p(out.ctypes.data)) != 0


def test_set_loss_takes_trunc_snr():
    vf = _model()
    key = vf.loss_key()
    vf.set_loss(weighting="trunc_snr")
    assert vf._loss == dict(penalty="mse", delta=1.0, weight_kind="trunc_snr", a=0.0, b=0.0) and vf.loss_key() != key
    vf.set_loss()
    assert vf._loss is None and vf.loss_key() == key


# ---- set_distill -------------------------------------------------------------------------------------------------------
def test_set_distill_argument_errors():
    from view_fusion_amd import UNet
    vf, teacher = _model(), _model()
    key = vf.loss_key()
    bad = [dict(teacher=teacher), dict(teacher=teacher, steps=0), dict(teacher=teacher, steps=11),
           dict(teacher=teacher, steps=2.0), dict(teacher=teacher, steps=True), dict(teacher=vf, steps=2),
           dict(teacher=teacher.denoise_fn, steps=2), dict(teacher=teacher, steps=2, guidance=-1.0),
           dict(teacher=teacher, steps=2, guidance=float("nan")), dict(teacher=teacher, steps=2, threshold=0.99),
           dict(teacher=teacher, steps=2, guidance=2.0, guidance_rescale=0.7), dict(teacher=None, steps=2),
           dict(teacher=_model(dict(SCHED, linear_end=0.08)), steps=2),
           dict(teacher=_model(dict(SCHED, num_timesteps=10)), steps=2),
           dict(teacher=_model(unet=dict(TINY, in_channel=9)), steps=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            vf.set_distill(**kw)
        assert vf._distill is None, kw                                  # a refused call leaves distillation off
    no_sched = type(vf)(UNet(**TINY), {"train": dict(SCHED)})
    with pytest.raises(ValueError, match="noise schedule"):
        vf.set_distill(no_sched, steps=2)
    # what is not built is refused, not half-built
    vf.set_cond_dropout(0.1)
    with pytest.raises(ValueError, match="conditioning dropout"):
        vf.set_distill(teacher, steps=2)
    vf.set_cond_dropout(0.0)
    vf.set_level_sampler("fixed", bins=4, probs=[1, 1, 1, 1])
    with pytest.raises(ValueError, match="level sampler"):
        vf.set_distill(teacher, steps=2)
    vf.set_level_sampler(None)
    assert vf.loss_key() != key
    # a teacher with another prediction and its own view weighting is fine; a zero-terminal-SNR eps teacher is not
    teacher.set_prediction("v")
    teacher.weighting_inference = False
    vf.set_distill(teacher, steps=4, guidance=2.0)
    assert vf._distill["steps"] == 4 and vf._distill["prediction"] == "v" and not teacher.training
    zt_s, zt_t = _model(SCHED_ZT), _model(SCHED_ZT)
    with pytest.raises(ValueError, match="zero terminal SNR|gamma = 0"):
        zt_s.set_distill(zt_t, steps=2)
    # a CPU model cannot run the step
    vf.train()
    y = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match="GPU"):
        vf(y_cond=y[:, None], view_count=[1], angle=torch.zeros(1, 1), y_0=y)
    k2 = vf.loss_key()
    vf.set_distill(None)
    assert vf._distill is None and vf.last_distill is None and vf.loss_key() not in (key, k2)


def test_the_teacher_stays_outside_the_module_tree():
    ref = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))["tiny"]
    vf, teacher = _model(), _model()
    before = [k for k, _ in vf.state_dict().items()]
    n_params, n_mods = len(list(vf.parameters())), len(list(vf.modules()))
    vf.set_distill(teacher, steps=5)
    assert [k for k, _ in vf.state_dict().items()] == before == [k for k, _ in ref]
    assert len(list(vf.parameters())) == n_params and len(list(vf.modules())) == n_mods
    mine = {id(p) for p in vf.parameters()}
    assert not any(id(p) in mine for p in teacher.parameters())
    assert all(m is not teacher and m is not teacher.denoise_fn for m in vf.modules())
    assert not any("distill" in n or "teacher" in n for n, _ in vf.named_buffers())
    assert not any("teacher" in n for n, _ in vf.named_modules())
    vf.train()                                                        # the student's mode does not reach the teacher
    assert not teacher.training and not teacher.denoise_fn.training
    vf.zero_grad()
    assert all(p.grad is None for p in teacher.parameters())
    assert len(torch.optim.Adam(vf.parameters()).param_groups[0]["params"]) == n_params


def test_checkpoint_carries_the_stage(tmp_path):
    from view_fusion_amd import drivers
    vf = _model()
    opt = torch.optim.Adam(vf.parameters())
    path = str(tmp_path / "stage.pt")
    drivers.save_checkpoint(path, vf, opt, it=3, distill=dict(steps=4), prediction=vf.prediction)
    extra = drivers.load_checkpoint(path, _model())
    assert extra["distill"] == dict(steps=4) and extra["it"] == 3
    for bad in (dict(steps=0), dict(steps=2.0), dict(K=4), 4):
        with pytest.raises(ValueError, match="distill"):
            drivers.save_checkpoint(path, vf, opt, distill=bad)
    drivers.save_checkpoint(path, vf, opt, it=1)
    assert "distill" not in drivers.load_checkpoint(path, _model())


def test_progressive_distill_argument_errors():
    from view_fusion_amd import drivers

    class _T:                                                         # argument checks come before any step
        module, opt = _model(), None

    for kw in (dict(start_steps=8, end_steps=3, iters_per_stage=1), dict(start_steps=4, end_steps=4, iters_per_stage=1),
               dict(start_steps=12, end_steps=2, iters_per_stage=1), dict(start_steps=32, end_steps=2, iters_per_stage=1),
               dict(start_steps=8, end_steps=2, iters_per_stage=0), dict(start_steps=8, end_steps=0, iters_per_stage=1),
               dict(start_steps=8, end_steps=2, iters_per_stage=1, from_ema=True)):
        with pytest.raises(ValueError):
            drivers.progressive_distill(_T(), _model(), [], **kw)
