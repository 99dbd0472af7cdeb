"""The variational bound at model level on the GPU (ViewFusion.bound_terms, drivers.bits_per_dim, drivers.evaluate(nll=True);
definition at the head of csrc/diffusion.hip) -- the TINY UNet of the other model-level tests with six and nine output
channels, T = 8, 16x16, B = 2, view counts (3, 2).

  1. wiring: bound_terms is tests/nll_ref.py fed the device's own UNet outputs (a forward hook), step by step, on the full
     chain and on sample_steps=3, for a fixed variance (small and large), a learned one, and a nine-channel network with
     the learned variance off (channels 6..8 ignored).  Tolerance: the kernel tolerance of tests/test_gpu_nll.py -- 4 x
     the float32 restatement's own distance from float64 over the chain's steps (every measured floor is nonzero).
     total_bpd == prior_bpd + vb.sum(1) and eps_mse == x0_mse g / (1 - g) to the bit; "large" differs from "small" only
     through lp: the same x0_mse, prior and decoder column, bit for bit.
  2. the cross-check against code that exists: for a nine-channel model and k >= 1, bound_terms(clip_denoised=False)'s
     vb[:, k] against the training KL of ops.compose_loss(vlb=) on the same UNet output with the level on gammas[k] (the
     training forward's level (g[t] - g[t-1]) u + g[t-1] need not land on the table value for any fp32 u, so the assertion
     is made at the op).  Both float64 restatements (nll_ref, vlb_ref) are evaluated: they agree up to the fp32 rounding
     of the level -- the training term forms kappa^2 = (1 - g) / g from the fp32 level, the bound reads the table pair
     made in float64, a relative 2^-24 / (1 - g).  Each device value is held to its own restatement by 4 x that
     restatement's float32 floor over the chain (bound_terms' vb as in the wiring test; the training KL likewise), and
     the two device values to each other by the sum of those two tolerances plus the distance of the restatements:
     nothing in a tolerance is measured from a device value.
  3. the refusals, before any launch.
  4. drivers.bits_per_dim with seed=: the noisy targets a sample's rows carry are the same bits under another batch
     size and order; the reduced numbers agree within the kernel tolerance.  evaluate(nll=True) adds "bpd";
     evaluate() returns today's keys.
Figures are printed before the assertions (run with -s); profiles/nll.md records them."""
import numpy as np
import pytest
import torch

import nll_ref
import vlb_ref
from conftest import TINY

pytestmark = pytest.mark.gpu
SCHED = dict(schedule="linear", num_timesteps=8, linear_start=1e-4, linear_end=0.09)
T = SCHED["num_timesteps"]
NINE = dict(TINY, out_channel=9)
VC = [3, 2]
B, HW = 2, (16, 16)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _model(dev, cfg=TINY, sched=SCHED):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**cfg)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": dict(sched)}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


@pytest.fixture(scope="module")
def models(dev):
    six, nine, nine_off = _model(dev), _model(dev, NINE), _model(dev, NINE)
    nine.set_learned_variance()
    return {"six": six, "nine": nine, "nine_off": nine_off}


@pytest.fixture(scope="module")
def batch(dev):
    g = torch.Generator().manual_seed(4)
    y_0 = torch.rand(B, 3, *HW, generator=g) * 2 - 1
    y_cond = torch.rand(B, max(VC), 3, *HW, generator=g) * 2 - 1
    angle = 2 * np.pi / 24 * torch.randint(0, 24, (B, 1), generator=g).float()
    noise = torch.randn(B, T, 3, *HW, generator=g)
    return dict(y_0=y_0.to(dev), y_cond=y_cond.to(dev), angle=angle.to(dev), noise=noise.to(dev))


def _hooked(vf, fn):
    """fn() with every (input, output) of the network kept, in call order."""
    calls = []
    h = vf.denoise_fn.register_forward_hook(lambda m, i, o: calls.append((i[0].detach().clone(), o.detach().clone())))
    try:
        return fn(), calls
    finally:
        h.remove()


def _tables32(vf, tau, fixed_variance="small"):
    from view_fusion_amd import schedule
    tab = schedule.nll_tables(vf.betas64, tau, vf.prediction, fixed_variance)
    return {k: v.astype(np.float32) for k, v in tab.items()}


def _rel(a, b):
    return float((np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)).max())


# ---- 1. wiring -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [None, 3])
@pytest.mark.parametrize("which,fixed", [("six", "small"), ("six", "large"), ("nine", "small"), ("nine_off", "small")])
def test_bound_terms_is_the_restatement_on_the_devices_own_outputs(dev, models, batch, which, fixed, steps):
    from view_fusion_amd import ops, schedule
    vf = models[which]
    learned = which == "nine"
    tau = np.arange(T) if steps is None else schedule.sample_timesteps(T, steps)
    K = len(tau)
    noise = batch["noise"][:, :K].contiguous()
    res, calls = _hooked(vf, lambda: vf.bound_terms(batch["y_cond"], VC, batch["angle"], batch["y_0"], noise=noise,
                                                    sample_steps=steps, fixed_variance=fixed))
    assert len(calls) == K and res["tau"].tolist() == tau.tolist()
    assert all(tuple(res[n].shape) == (B, K) for n in ("vb", "x0_mse", "eps_mse")) and res["total_bpd"].shape == (B,)
    tab = _tables32(vf, None if steps is None else tau, fixed)
    gam = vf.gammas.cpu().numpy()
    y_0 = batch["y_0"].cpu().numpy()
    tau_d = torch.from_numpy(tau.astype(np.int64)).to(dev)
    rec = []
    for k in range(K):
        x, out = calls[K - 1 - k]                                    # the loop runs k = K-1 ... 0
        kidx = torch.full((B,), k, device=dev, dtype=torch.int64)
        y_k = ops.nll_noisy(batch["y_0"], kidx, tau_d, vf.gammas, noise=noise)
        assert torch.equal(x[0, 3:6], y_k[0]) and torch.equal(x[VC[0], 3:6], y_k[1])     # what the network was shown
        row = tuple(tab[n][k] for n in ("a", "b", "c0", "hi", "lo"))
        args = (out.cpu().numpy(), VC, True, y_k.cpu().numpy(), y_0, row)
        kw = dict(learned=learned, decoder=k == 0, large=fixed == "large")
        r64, r32 = nll_ref.term(*args, **kw), nll_ref.term(*args, **kw, dt=np.float32)
        for name in ("vb", "x0_mse"):
            rec.append((name, k, _rel(res[name][:, k].cpu().numpy(), r64[name]), _rel(r32[name], r64[name])))
    for name in ("vb", "x0_mse"):
        mine = [r for r in rec if r[0] == name]
        floor = max(r[3] for r in mine)
        print(f"{which} {fixed} K={K} {name}: fp32 restatement floor {floor:.2e}, device worst {max(r[2] for r in mine):.2e}; "
              f"vb {res['vb'][0].cpu().numpy()}")
        assert floor > 0 and all(r[2] <= 4.0 * floor for r in mine), mine
    # the prior is the op (held to float64 in tests/test_gpu_nll.py) on the targets and the model's own gammas, to the bit
    p64, p32 = nll_ref.prior(y_0, gam[-1]), nll_ref.prior(y_0, gam[-1], np.float32)
    print(f"prior: fp32 restatement {_rel(p32, p64):.2e}, device {_rel(res['prior_bpd'].cpu().numpy(), p64):.2e}")
    assert torch.equal(res["prior_bpd"], ops.nll_prior(batch["y_0"], vf.gammas))
    assert torch.equal(res["total_bpd"], res["prior_bpd"] + res["vb"].sum(dim=1))
    g = vf.gammas[tau_d].double()
    assert torch.equal(res["eps_mse"], res["x0_mse"] * (g / (1.0 - g)).float())
    assert torch.isfinite(res["total_bpd"]).all()


def test_large_differs_from_small_only_through_lp(models, batch):
    vf = models["six"]
    args = (batch["y_cond"], VC, batch["angle"], batch["y_0"])
    small = vf.bound_terms(*args, noise=batch["noise"])
    large = vf.bound_terms(*args, noise=batch["noise"], fixed_variance="large")
    again = vf.bound_terms(*args, noise=batch["noise"])
    assert all(torch.equal(small[k], again[k]) for k in small)                       # the same bits on every run
    assert torch.equal(small["x0_mse"], large["x0_mse"]) and torch.equal(small["prior_bpd"], large["prior_bpd"])
    assert torch.equal(small["vb"][:, 0], large["vb"][:, 0])                         # the decoder row is lo_dec in both
    assert not torch.equal(small["vb"][:, 1:], large["vb"][:, 1:])
    # without the clamp y0 moves, and with it everything but the prior
    raw = vf.bound_terms(*args, noise=batch["noise"], clip_denoised=False)
    assert torch.equal(raw["prior_bpd"], small["prior_bpd"]) and not torch.equal(raw["x0_mse"], small["x0_mse"])
    # unseeded and seeded draws run too; a seeded evaluation is a function of (seed, ids)
    s1 = vf.bound_terms(*args, seed=9, sample_ids=[4, 1])
    s2 = vf.bound_terms(*args, seed=9, sample_ids=[4, 1])
    s3 = vf.bound_terms(*args, seed=10, sample_ids=[4, 1])
    assert torch.equal(s1["vb"], s2["vb"]) and not torch.equal(s1["vb"], s3["vb"])
    assert torch.isfinite(vf.bound_terms(*args)["total_bpd"]).all()


def test_training_mode_is_left_as_it_was_and_dropout_is_off(dev, batch):
    vf = _model(dev, dict(TINY, dropout=0.2))
    ref = _model(dev, dict(TINY, dropout=0.0))
    vf.train()
    args = (batch["y_cond"], VC, batch["angle"], batch["y_0"])
    a = vf.bound_terms(*args, noise=batch["noise"])
    assert vf.training and vf.denoise_fn.training
    assert torch.equal(a["vb"], ref.bound_terms(*args, noise=batch["noise"])["vb"])  # the inference path: no Dropout


# ---- 2. the cross-check against the training KL ------------------------------------------------------------------------------------
def test_vb_is_the_training_kl_at_the_table_level(dev, models, batch):
    from view_fusion_amd import ops
    vf = models["nine"]
    res, calls = _hooked(vf, lambda: vf.bound_terms(batch["y_cond"], VC, batch["angle"], batch["y_0"], noise=batch["noise"],
                                                    clip_denoised=False))
    off, _, _ = ops.view_offsets(VC, dev)
    c1, hi, lo = vf._lv_tables()
    tab = _tables32(vf, None)
    gam = vf.gammas.cpu().numpy()
    y_0, noise = batch["y_0"].cpu().numpy(), batch["noise"].cpu().numpy()
    rec = []
    for k in range(1, T):
        out = calls[T - 1 - k][1]
        level = vf.gammas[k].expand(B).contiguous()
        t = torch.full((B,), k, device=dev, dtype=torch.int64)
        got = ops.compose_loss(out, batch["noise"][:, k].contiguous(), off, B, True, level, vlb=(t, c1, hi, lo, 1.0))
        kl_train = got[2].cpu().numpy().astype(np.float64)
        vb = res["vb"][:, k].cpu().numpy().astype(np.float64)
        row = tuple(tab[n][k] for n in ("a", "b", "c0", "hi", "lo"))
        assert row[2] == c1[k].item() and row[3] == hi[k].item() and row[4] == lo[k].item()    # the same table values
        o = out.cpu().numpy()
        a_args = dict(learned=True, clip=False)
        ref_a = nll_ref.term(o, VC, True, nll_ref.noisy(y_0, noise[:, k], gam[k]), y_0, row, **a_args)["vb"]
        ref_a32 = nll_ref.term(o, VC, True, nll_ref.noisy(y_0, noise[:, k], gam[k], np.float32), y_0, row, **a_args,
                               dt=np.float32)["vb"]
        b_args = (o, noise[:, k], None, VC, True, np.full(B, gam[k], dtype=np.float32), [k] * B, c1.cpu().numpy(),
                  hi.cpu().numpy(), lo.cpu().numpy(), 1.0)
        ref_b = vlb_ref.hybrid(*b_args)["sample_vlb"]
        ref_b32 = vlb_ref.hybrid(*b_args, dtype=np.float32)["sample_vlb"]
        refs = _rel(ref_a, ref_b)
        level_rounding = 4.0 * 2.0 ** -24 / (1.0 - float(gam[k])) + 1e-6
        print(f"k {k}: vb {vb}  training KL {kl_train}  |diff| {np.abs(vb - kl_train).max():.2e}  rel distances from float64: "
              f"vb {_rel(vb, ref_a):.2e} (fp32 restatement {_rel(ref_a32, ref_a):.2e})  KL {_rel(kl_train, ref_b):.2e} "
              f"(fp32 restatement {_rel(ref_b32, ref_b):.2e})  restatements apart {refs:.2e} (level rounding "
              f"{level_rounding:.2e})")
        assert refs <= level_rounding
        rec.append((k, vb, kl_train, ref_a, ref_b, _rel(ref_a32, ref_a), _rel(ref_b32, ref_b)))
    floor_a, floor_b = max(r[5] for r in rec), max(r[6] for r in rec)   # over the chain's steps, as in the wiring test
    print(f"fp32 restatement floors over the chain: bound_terms' vb {floor_a:.2e}, the training KL {floor_b:.2e}")
    assert floor_a > 0 and floor_b > 0
    for k, vb, kl_train, ref_a, ref_b, _, _ in rec:
        tol_a, tol_b = 4.0 * floor_a * np.abs(ref_a), 4.0 * floor_b * np.abs(ref_b)
        assert np.all(np.abs(vb - ref_a) <= tol_a), (k, vb, ref_a, floor_a)
        assert np.all(np.abs(kl_train - ref_b) <= tol_b), (k, kl_train, ref_b, floor_b)
        assert np.all(np.abs(vb - kl_train) <= tol_a + tol_b + np.abs(ref_a - ref_b)), k


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_launch(dev, models, batch):
    from view_fusion_amd import _lib
    args = (batch["y_cond"], VC, batch["angle"], batch["y_0"])
    zero = _model(dev, TINY, dict(SCHED, zero_terminal_snr=True))
    sc = _model(dev)
    sc.set_self_cond(0.5)
    n0 = _lib.N_CALLS
    vf = models["six"]
    for kw in (dict(guidance=2.0), dict(threshold=0.9), dict(guidance=2.0, guidance_rescale=0.5),
               dict(fixed_variance="medium"), dict(sample_steps=T + 1), dict(noise=batch["noise"][:, :3].contiguous())):
        with pytest.raises(ValueError):
            vf.bound_terms(*args, **kw)
    with pytest.raises(ValueError, match="self-conditioned"):
        sc.bound_terms(*args)
    with pytest.raises(ValueError, match="large"):
        models["nine"].bound_terms(*args, fixed_variance="large")
    with pytest.raises(ValueError, match="GPU"):
        vf.bound_terms(batch["y_cond"].cpu(), VC, batch["angle"].cpu(), batch["y_0"].cpu())
    with pytest.raises(ValueError, match="gamma = 0"):
        zero.bound_terms(*args)
    six_lv = _model(dev)
    six_lv.set_learned_variance()
    with pytest.raises(ValueError, match="out_channel = 6"):
        six_lv.bound_terms(*args)
    # ... and through evaluate(nll=True): before its first generate() launches anything
    from view_fusion_amd import drivers
    b = [dict(target=batch["y_0"], cond=batch["y_cond"], angle=batch["angle"], view_count=torch.tensor(VC))]
    with pytest.raises(ValueError, match="self-conditioned"):
        drivers.evaluate(sc, b, nll=True)
    with pytest.raises(ValueError, match="out_channel = 6"):
        drivers.evaluate(six_lv, b, nll=True)
    assert _lib.N_CALLS == n0
    # v-prediction on the zero-terminal-SNR schedule runs, and its prior is exactly 0
    zero.set_prediction("v")
    res = zero.bound_terms(*args, noise=batch["noise"])
    assert torch.isfinite(res["total_bpd"]).all() and not res["prior_bpd"].any()


# ---- 4. the drivers -------------------------------------------------------------------------------------------------------------------
def _targets_shown(vf, fn, counts):
    """fn() -> (its result, per call the noisy target of every sample: channels 3..5 of its first stacked row)."""
    res, calls = _hooked(vf, fn)
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    return res, [x[first.tolist(), 3:6].cpu().numpy() for x, _ in calls]


def test_bits_per_dim_does_not_depend_on_the_batching(dev, models, batch):
    from view_fusion_amd import drivers
    vf = models["six"]
    whole = [dict(target=batch["y_0"], cond=batch["y_cond"], angle=batch["angle"], view_count=VC, ids=torch.tensor([7, 3]))]
    parts = [dict(target=batch["y_0"][i:i + 1], cond=batch["y_cond"][i:i + 1], angle=batch["angle"][i:i + 1],
                  view_count=VC[i:i + 1], ids=torch.tensor([[7, 3][i]])) for i in (1, 0)]
    a, shown_a = _targets_shown(vf, lambda: drivers.bits_per_dim(vf, whole, seed=5), VC)
    b, shown_b = _targets_shown(vf, lambda: drivers.bits_per_dim(vf, parts, seed=5), [1])
    assert set(a) == {"bpd", "prior_bpd", "vb", "x0_mse", "eps_mse"} and a["vb"].shape == (T,) and a["bpd"].dim() == 0
    assert len(shown_a) == T and len(shown_b) == 2 * T
    for j in range(T):                                               # parts: sample 1's chain first, then sample 0's
        assert np.array_equal(shown_a[j][1], shown_b[j][0]) and np.array_equal(shown_a[j][0], shown_b[T + j][0])
    # the tolerance of the reduced numbers: the float32 restatement's floor over the chain, as in the wiring test
    res, calls = _hooked(vf, lambda: vf.bound_terms(batch["y_cond"], VC, batch["angle"], batch["y_0"], seed=5,
                                                    sample_ids=[7, 3]))
    tab = _tables32(vf, None)
    floor = 0.0
    for k in range(T):
        x, out = calls[T - 1 - k]
        y_k = x[[0, VC[0]], 3:6].cpu().numpy()
        row = tuple(tab[n][k] for n in ("a", "b", "c0", "hi", "lo"))
        args = (out.cpu().numpy(), VC, True, y_k, batch["y_0"].cpu().numpy(), row)
        r64, r32 = nll_ref.term(*args, decoder=k == 0), nll_ref.term(*args, decoder=k == 0, dt=np.float32)
        floor = max(floor, _rel(r32["vb"], r64["vb"]))
    tol = 4.0 * floor
    assert floor > 0
    assert torch.equal(a["bpd"], res["total_bpd"].mean())
    for name in ("bpd", "prior_bpd", "vb", "x0_mse", "eps_mse"):
        e = _rel(b[name].cpu().numpy(), a[name].double().cpu().numpy())
        print(f"bits_per_dim {name}: one batch of 2 against two of 1, reversed: rel {e:.2e} (tolerance {tol:.2e})")
        assert e <= tol, name
    # a strided chain and the other options reach bound_terms
    c = drivers.bits_per_dim(vf, whole, seed=5, sample_steps=3, fixed_variance="large", clip_denoised=False)
    assert c["vb"].shape == (3,) and torch.isfinite(c["bpd"])


def test_evaluate_reports_bpd_only_when_asked(dev):
    from view_fusion_amd import _lib, drivers
    vf = _model(dev, TINY, dict(SCHED, num_timesteps=10))             # generate() wants T > its 8 snapshots
    g = torch.Generator().manual_seed(6)
    batches = [dict(target=(torch.rand(B, 3, *HW, generator=g) * 2 - 1).to(dev),
                    cond=(torch.rand(B, 3, 3, *HW, generator=g) * 2 - 1).to(dev),
                    angle=torch.rand(B, 1, generator=g).to(dev), view_count=torch.tensor(VC), ids=torch.tensor([0, 1]))]
    n0 = _lib.N_CALLS
    plain = drivers.evaluate(vf, batches, seed=3, use_graph=False)
    n1 = _lib.N_CALLS
    again = drivers.evaluate(vf, batches, seed=3, use_graph=False)
    n2 = _lib.N_CALLS
    with_nll = drivers.evaluate(vf, batches, seed=3, use_graph=False, nll=True)
    assert set(plain) == {"psnr"} and set(with_nll) == {"psnr", "bpd"}
    assert n2 - n1 <= n1 - n0                                          # (the first call may pack weights)
    assert torch.equal(plain["psnr"], with_nll["psnr"]) and torch.equal(plain["psnr"], again["psnr"])
    want = drivers.bits_per_dim(vf, batches, seed=3)["bpd"]
    assert torch.equal(with_nll["bpd"], want)
