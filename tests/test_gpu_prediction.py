"""v- and x0-prediction on the GPU (ViewFusion.set_prediction, ops.compose_loss(prediction=, y_0=); the
compose_loss_fwd / _finish / _bwd kernels of csrc/diffusion.hip under PRED = v | x0; definition at the head of that file,
weights in csrc/loss_weight.h) against the float64 restatement tests/prediction_ref.py.

  1. loss and d unet_out against float64: "v" and "x0" x every penalty x every weighting, softmax and mean, at the shapes
     of test_gpu_loss_options.py for the reasons it gives (8x8: fewer float4s than one workgroup; 12x20: n4 % 256 != 0;
     128x192 at B = 1: more than 64 * 256 float4s, the grid-stride loop and all 64 partials), and with its tolerances:
     close() (1e-6 relative + 1e-7) on loss and per-sample loss, d unet_out max-relative < 1e-5.  The wanted target is
     noise_hat - sign (0.01 + |N|) as there; the noise is drawn freely and y_0 solved from it in float64 and rounded to
     fp32; the float64 reference reads those fp32 inputs, so min |d| >= 1e-3 is asserted and no element is excluded.
     Measured on the device (profiles/prediction.md): loss rel <= 1.9e-7, sample loss rel <= 1.7e-7, dout rel <= 1.0e-6.
  2. the native weights the device hands back (want_weight=True) against the host mirror and float64, within close() -- the
     tolerance the loss-options test applies to the quantities that carry the eps weights;
  3. the default is untouched: set_prediction("eps") against a model that never called it, bit for bit, on the same
     launches; _sched() hands out the buffers themselves;
  4. the tails with v / x0 table pairs against the restatement (the tolerance of test_gpu_sampler_steps.py, rel 2e-5), x0's
     y0_hat == out to the bit, and the three-launch tail (guidance + rescale, threshold);
  5. model level: forward() under "v" against ops.compose_loss on an explicitly built fp32 target; generate() under "v"
     (dpmpp2m K = 4, the ancestral chain) against the float64 chain through the oracle UNet (max-abs 1e-3, the
     sampler-steps test's chain tolerance); the same on a zero-terminal-SNR schedule: finite;
  6. Trainer: "v" + min_snr + loss_bins + a fixed level sampler, graph replay == eager bit for bit, accum_steps = 2, and
     set_prediction("x0") after the capture.
Figures are printed before the assertions (run with -s)."""
import numpy as np
import pytest
import torch

import loss_ref
import prediction_ref
import threshold_ref
from conftest import TINY

pytestmark = pytest.mark.gpu
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
T = SCHED["num_timesteps"]
WEIGHT_CASES = [(None, 0.0, 0.0), ("min_snr", 5.0, 0.0), ("p2", 1.0, 1.0)]
DELTA = 0.7
SHAPES = {"8x8": ((8, 8), (1, 3, 2)), "12x20": ((12, 20), (1, 3, 2)), "128x192": ((128, 192), (2,))}
LEVELS = {3: [0.95, 0.4, 0.05], 1: [0.95]}
PREDS = ("v", "x0")
KERNEL_RTOL, CHAIN_TOL = 2e-5, 1e-3          # test_gpu_sampler_steps.py: one kernel (max|a-b| / max|b|), a chain (max-abs)
VC = [1, 3, 2]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def rel(a, b):
    a, b = (torch.as_tensor(x).detach().double().cpu().numpy() for x in (a, b))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def close(a, b):
    """test_gpu_loss_options.py's loss tolerance, element by element."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) < 1e-6 * np.abs(b) + 1e-7))


_INPUTS = {}


def _inputs(shape, weighting, prediction):
    """Fixed-seed unet_out / noise / y_0 / level of one shape, built once and left unchanged: the wanted target is
    noise_hat - d with |d| = 0.01 + |N(0, 1)| and a random sign (test_gpu_loss_options.py's construction, the same
    generator), then the noise from the same generator and y_0 = (sqrt(g) noise - target) / sqrt(1 - g) in float64,
    rounded to fp32 (x0: y_0 = the target)."""
    key = (shape, weighting, prediction)
    if key not in _INPUTS:
        (H, W), vc = SHAPES[shape]
        g = torch.Generator().manual_seed(3)
        out = (torch.randn(sum(vc), 6, H, W, generator=g) * 2).numpy()
        nh, _ = loss_ref.compose(out, vc, weighting)
        mag = 0.01 + torch.randn(len(vc), 3, H, W, generator=g).abs().double().numpy()
        sign = np.where(torch.rand(len(vc), 3, H, W, generator=g).numpy() < 0.5, -1.0, 1.0)
        want = nh - sign * mag
        noise = torch.randn(len(vc), 3, H, W, generator=g).numpy()
        level = np.array(LEVELS[len(vc)], dtype=np.float32)
        lv = level.astype(np.float64).reshape(-1, 1, 1, 1)
        y_0 = want if prediction == "x0" else (np.sqrt(lv) * noise.astype(np.float64) - want) / np.sqrt(1.0 - lv)
        _INPUTS[key] = (out, noise, y_0.astype(np.float32), level, vc)
    return _INPUTS[key]


def _run_op(dev, out, noise, y_0, level, vc, weighting, prediction, penalty, kind, a, b, gloss=1.7, **kw):
    from view_fusion_amd import ops
    off, S, _ = ops.view_offsets(list(vc), dev)
    og = torch.from_numpy(out).to(dev).requires_grad_(True)
    loss, sl, w = ops.compose_loss(og, torch.from_numpy(noise).to(dev), off, len(vc), weighting,
                                   torch.from_numpy(level).to(dev), penalty, DELTA, kind, a, b, want_weight=True,
                                   prediction=prediction, y_0=torch.from_numpy(y_0).to(dev), **kw)
    assert not sl.requires_grad and not w.requires_grad and loss.requires_grad
    (loss * gloss).backward()
    return float(loss.detach()), sl.cpu().numpy(), og.grad.cpu().numpy(), w.cpu().numpy()


# ---- 1. / 2. op level --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_compose_loss_against_float64(dev, shape, weighting):
    """Measured over both predictions, all penalties and weightings: loss rel <= 1.9e-7, sample_loss rel <= 1.7e-7,
    dout rel <= 1.0e-6 (profiles/prediction.md has the figure of every shape)."""
    failures, worst = [], [0.0, 0.0, 0.0]
    for prediction in PREDS:
        out, noise, y_0, level, vc = _inputs(shape, weighting, prediction)
        n4 = 3 * out.shape[2] * out.shape[3] // 4
        assert (n4 < 256) if shape == "8x8" else (n4 > 64 * 256) if shape == "128x192" else (n4 % 256 != 0)
        for penalty in loss_ref.PENALTIES:
            for kind, a, b in WEIGHT_CASES:
                ref = prediction_ref.loss(out, noise, y_0, vc, weighting, level, prediction, penalty, DELTA, kind, a, b,
                                          gloss=1.7)
                assert np.abs(ref["d"]).min() >= 1e-3                  # L1: no element near the kink, none excluded
                if penalty == "huber":
                    frac = float((np.abs(ref["d"]) <= DELTA).mean())
                    assert 0.1 < frac < 0.9, frac                      # both branches
                loss, sl, dout, _ = _run_op(dev, out, noise, y_0, level, vc, weighting, prediction, penalty, kind, a, b)
                e_loss = abs(loss - ref["loss"]) / abs(ref["loss"])
                e_sl = float((np.abs(sl - ref["sample_loss"]) / np.abs(ref["sample_loss"])).max())
                e_d = rel(dout, ref["dout"])
                worst = [max(x, y) for x, y in zip(worst, (e_loss, e_sl, e_d))]
                print(f"{shape} softmax={weighting} {prediction:2s} {penalty:5s} {str(kind):7s}: loss {loss:.9g} "
                      f"(f64 {ref['loss']:.12g}) rel {e_loss:.2e}  sample_loss rel {e_sl:.2e}  dout rel {e_d:.2e}")
                if not (close(loss, ref["loss"]) and close(sl, ref["sample_loss"]) and e_d < 1e-5):
                    failures.append((prediction, penalty, kind, e_loss, e_sl, e_d))
                if len(vc) > 1:
                    assert np.all(dout[0, 3:] == 0), (prediction, penalty, kind)   # one view: zero logit gradient
                if not weighting:
                    assert np.all(dout[:, 3:] == 0)
    print(f"{shape} softmax={weighting}: worst loss rel {worst[0]:.2e}  sample_loss rel {worst[1]:.2e}  dout rel {worst[2]:.2e}")
    assert not failures, failures


@pytest.mark.parametrize("prediction", PREDS)
def test_native_weights_on_the_device(dev, prediction):
    """The third output of compose_loss: the prediction's native weight alone, also next to a per-sample scale."""
    from view_fusion_amd import ops
    out, noise, y_0, level, vc = _inputs("8x8", True, prediction)
    scale = np.array([0.5, 2.0, 1.25], dtype=np.float32)
    for kind, a, b in WEIGHT_CASES:
        host = ops.loss_weights_pred_host(level, prediction, kind, a, b).numpy()
        w64 = prediction_ref.weights(level, prediction, kind, a, b)
        loss, sl, _, w = _run_op(dev, out, noise, y_0, level, vc, True, prediction, "mse", kind, a, b)
        loss_s, sl_s, _, w_s = _run_op(dev, out, noise, y_0, level, vc, True, prediction, "mse", kind, a, b,
                                       sample_scale=torch.from_numpy(scale).to(dev))
        e64 = float((np.abs(w - w64) / np.abs(w64)).max())
        print(f"{prediction} {kind}: device {w}  host {host}  f64 {w64}  |device - f64| rel {e64:.2e}  "
              f"device == host {np.array_equal(w, host)}")
        assert close(w, w64) and close(w, host)
        assert np.array_equal(w_s, w) and np.array_equal(sl_s, sl)       # the scale touches neither of them
        assert close(loss, float((w64 * sl.astype(np.float64)).mean()))
        assert close(loss_s, float((w64 * scale * sl.astype(np.float64)).mean()))
        if kind is None:
            assert (w == 1).all()
    # eps through the same public call is the existing path (and refuses y_0)
    _, _, w_eps = ops.compose_loss(torch.from_numpy(out).to(dev), torch.from_numpy(noise).to(dev),
                                   ops.view_offsets(list(vc), dev)[0], 3, True, torch.from_numpy(level).to(dev),
                                   weight_kind="min_snr", a=5.0, want_weight=True, prediction="eps")
    assert close(w_eps.cpu().numpy(), loss_ref.weights(level, "min_snr", 5.0))


def test_histogram_and_launches_of_the_prediction_path(dev):
    """The same two launches forward and one backward; the histogram receives the unweighted native per-sample loss."""
    from view_fusion_amd import ops
    out, noise, y_0, level, vc = _inputs("12x20", True, "v")
    Kb = 5
    hist = (torch.zeros(Kb, device=dev), torch.zeros(Kb, device=dev, dtype=torch.int32))
    ops.st.KERNEL_LOG = []
    try:
        _, sl, _, _ = _run_op(dev, out, noise, y_0, level, vc, True, "v", "huber", "min_snr", 5.0, 0.0, hist=hist)
        names = [r[5] for r in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None
    assert names == ["vf_compose_loss_pred_fwd", "vf_compose_loss_pred_bwd"]
    s, c = loss_ref.histogram(level, sl, Kb)
    assert np.array_equal(hist[1].cpu().numpy(), c) and c.sum() == 3
    assert np.all(np.abs(hist[0].cpu().numpy() - s) <= 4 * 2.0 ** -24 * np.abs(s))


# ---- 3. the default is untouched -----------------------------------------------------------------------------------------
def _model(dev, sched=SCHED):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": dict(sched)}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


def _batch(dev, B, vc, s=0):
    from view_fusion_amd import train
    return dict(train.synthetic_batch(B, 3, 16, dev, seed=40 + s), view_count=torch.tensor(vc))


def _inject(dev, B):
    g = torch.Generator().manual_seed(1)
    return dict(t=torch.tensor([15, 3, 9])[:B].to(dev), u=torch.rand(B, 1, generator=g).to(dev),
                noise=torch.randn(B, 3, 16, 16, generator=g).to(dev))


@pytest.mark.parametrize("objective", [dict(), dict(weighting="min_snr")], ids=["default", "min_snr"])
def test_eps_is_the_untouched_path(dev, objective):
    from view_fusion_amd import ops
    B = 3
    batch, inj = _batch(dev, B, VC), _inject(dev, B)
    runs = []
    for touch in (False, True):
        vf = _model(dev)
        vf.set_loss(**objective)
        if touch:
            vf.set_prediction("v")
            vf.set_prediction("eps")
        ops.st.KERNEL_LOG = []
        try:
            loss = vf(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"], **inj)
            loss.backward()
            names = [r[5] for r in ops.st.KERNEL_LOG]
        finally:
            ops.st.KERNEL_LOG = None
        runs.append((loss.detach().cpu(), [p.grad.cpu() for p in vf.parameters()], names))
        sched = vf._sched()
        assert all(sched[k].data_ptr() == getattr(vf, k).data_ptr() and sched[k] is getattr(vf, k) for k in sched)
    (la, ga, na), (lb, gb, nb) = runs
    assert torch.equal(la, lb) and all(torch.equal(x, y) for x, y in zip(ga, gb))
    assert na == nb and not [n for n in na if "_pred_" in n]
    assert ("vf_compose_loss_fwd" in na) == bool(objective) and ("vf_compose_fwd" in na) == (not objective)


# ---- 4. the tails ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vf(dev):
    return _model(dev)


def _tail_inputs(H, W, null_rows=False):
    g = torch.Generator().manual_seed(17 + H)
    out = torch.randn(sum(VC) + (3 if null_rows else 0), 6, H, W, generator=g) * 2
    y, z, prev = (torch.randn(3, 3, H, W, generator=g) for _ in range(3))
    return out, y, z, prev


@pytest.mark.parametrize("prediction", PREDS)
@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("H,W", [(8, 8), (12, 20)])
def test_tails_against_the_restatement(vf, dev, H, W, weighting, prediction):
    from oracle import view_fusion_ref as vfr
    from view_fusion_amd import ops, schedule
    B, K = 3, 5
    betas = vfr.beta_schedule(**SCHED)
    vf.set_prediction(prediction)
    try:
        sched = vf._sched()
        sched_cpu = {k: getattr(vf, k).cpu() for k in schedule.BUFFER_NAMES}
        out, y, z, prev = _tail_inputs(H, W)
        off, S, max_v = ops.view_offsets(VC, dev)
        comp, _, _ = vfr.compose(out.double(), VC, weighting)
        comp, y64, z64, prev64 = comp.numpy(), y.double().numpy(), z.double().numpy(), prev.double().numpy()
        out_d, y_d, z_d = out.to(dev), y.to(dev), z.to(dev)
        worst = 0.0
        for t in (T - 1, 4, 0):                                       # the ancestral tail, with the mean
            tt = torch.full((B,), t, device=dev)
            got, mean, _ = ops.p_sample_tail(out_d, off, y_d, z_d, tt, sched, B, max_v, weighting, want_mean=True)
            want, want_m, _, _ = prediction_ref.ancestral_step(sched_cpu, betas, prediction, t, y64, comp, z64)
            errs = (rel(got, want), rel(mean, want_m))
            worst = max(worst, *errs)
            print(f"{prediction} ancestral {H}x{W} weighting {weighting} t {t}: y_next rel {errs[0]:.2e}  mean rel {errs[1]:.2e}")
            assert torch.isfinite(got).all() and max(errs) <= KERNEL_RTOL
        tau = schedule.sample_timesteps(T, K)
        nan = torch.full((B, 3, H, W), float("nan"))
        for solver, eta in (("ddim", 0.0), ("ddim", 0.5), ("dpmpp2m", 0.0)):
            plan = vf._sampler_plan(tau.tolist(), solver, eta, dev)
            for k in range(K):
                second = solver == "dpmpp2m" and 0 < k < K - 1
                hist0 = prev if second else nan                        # a first-order step may find anything there
                want, want_y0, _ = prediction_ref.sampler_step(betas, tau, solver, eta, prediction, k, y64, comp,
                                                               hist0.double().numpy(), z64)
                hist = hist0.to(dev)
                got, _ = ops.sampler_step(out_d, off, y_d, z_d, torch.full((B,), k, device=dev), plan, B, max_v, weighting,
                                          y0_prev=hist)
                errs = (rel(got, want), rel(hist, want_y0))
                worst = max(worst, *errs)
                print(f"{prediction} {solver} eta {eta} {H}x{W} weighting {weighting} k {k}: y_new rel {errs[0]:.2e}  "
                      f"y0 rel {errs[1]:.2e}")
                assert torch.isfinite(got).all() and max(errs) <= KERNEL_RTOL
        print(f"{prediction} {H}x{W} weighting {weighting}: worst rel against the float64 restatement {worst:.2e}")
    finally:
        vf.set_prediction("eps")


@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("H,W", [(8, 8), (12, 20)])
def test_x0_tables_hand_the_composition_through_to_the_bit(vf, dev, H, W, weighting):
    """a = 0, b = -1: y0_hat == out exactly.  Ancestral, clip=False: the returned mean is fl(c1 compose + c2 y) of the
    composition ops.compose gives, with the tails' rounding (csrc/diffusion.hip, posterior_update): c1 compose rounded,
    then one fused multiply-add with c2 y -- restated here in float64, where c2 y is exact.  Few-step: the history
    buffer receives clamp(compose, -1, 1) itself."""
    from view_fusion_amd import ops, schedule
    B = 3
    out, y, z, _ = _tail_inputs(H, W)
    off, S, max_v = ops.view_offsets(VC, dev)
    out_d, y_d = out.to(dev), y.to(dev)
    comp, _ = ops.compose(out_d, off, B, max_v, weighting, want_weights=False)
    vf.set_prediction("x0")
    try:
        sched = vf._sched()
        for t in (T - 1, 4, 0):
            tt = torch.full((B,), t, device=dev)
            _, mean, _ = ops.p_sample_tail(out_d, off, y_d, None, tt, sched, B, max_v, weighting, clip=False, want_mean=True)
            c1 = np.float32(vf.posterior_mean_coef1[t].item())
            c2 = np.float64(np.float32(vf.posterior_mean_coef2[t].item()))
            p = (c1 * comp.cpu().numpy()).astype(np.float32)            # one fp32 rounding
            want = (c2 * y.numpy().astype(np.float64) + p.astype(np.float64)).astype(np.float32)
            assert np.array_equal(mean.cpu().numpy(), want), (t, float(np.abs(mean.cpu().numpy() - want).max()))
        tau = schedule.sample_timesteps(T, 5).tolist()
        plan = vf._sampler_plan(tau, "dpmpp2m", 0.0, dev)
        hist = torch.full((B, 3, H, W), float("nan"), device=dev)
        ops.sampler_step(out_d, off, y_d, None, torch.full((B,), 4, device=dev), plan, B, max_v, weighting, y0_prev=hist)
        assert torch.equal(hist, comp.clamp(-1.0, 1.0))
    finally:
        vf.set_prediction("eps")


@pytest.mark.parametrize("prediction", PREDS)
def test_three_launch_tail_with_other_tables(vf, dev, prediction):
    """Guidance 2.0 + guidance_rescale 0.7 (sigma of the composed output in the network's own parameterisation) through
    the ancestral tail, threshold 0.9 through the few-step tail: threshold_ref's functions on the prediction's y0_hat."""
    from oracle import view_fusion_ref as vfr
    from view_fusion_amd import ops, schedule
    B, H, W, K = 3, 12, 20, 5
    betas = vfr.beta_schedule(**SCHED)
    out, y, z, prev = _tail_inputs(H, W, null_rows=True)
    off, S, max_v = ops.view_offsets(VC, dev)
    out_d, y_d, z_d = out.to(dev), y.to(dev), z.to(dev)
    y64, z64, prev64 = y.double().numpy(), z.double().numpy(), prev.double().numpy()
    vf.set_prediction(prediction)
    try:
        sched_cpu = {k: getattr(vf, k).cpu() for k in schedule.BUFFER_NAMES}
        comp_g, _, r = threshold_ref.composed_eps(out.double(), VC, True, 2.0, 0.7)
        gs = ops.guidance_scales(dev, B, 2.0)
        ops.st.KERNEL_LOG = []
        try:
            for t in (T - 1, 4):
                tt = torch.full((B,), t, device=dev)
                got, mean, _ = ops.p_sample_tail(out_d, off, y_d, z_d, tt, vf._sched(), B, max_v, True, want_mean=True,
                                                 guidance=gs, S=S, guidance_rescale=0.7)
                want, want_m, _, _ = prediction_ref.ancestral_step(sched_cpu, betas, prediction, t, y64, comp_g, z64)
                errs = (rel(got, want), rel(mean, want_m))
                print(f"{prediction} guided 2.0 rescale 0.7 (r {r}) t {t}: y_next rel {errs[0]:.2e}  mean rel {errs[1]:.2e}")
                assert max(errs) <= KERNEL_RTOL
            names = [e[5] for e in ops.st.KERNEL_LOG]
        finally:
            ops.st.KERNEL_LOG = None
        assert names == ["vf_compose_eps", "vf_sample_stat", "vf_p_sample_tail_eps"] * 2
        assert (np.abs(r - 1.0) > 1e-3).all()                          # (the rescale does something)
        comp, _, _ = threshold_ref.composed_eps(out[:S].double(), VC, True)
        tau = schedule.sample_timesteps(T, K)
        plan = vf._sampler_plan(tau.tolist(), "dpmpp2m", 0.0, dev)
        out_c = out_d[:S].contiguous()
        scales = []
        for k in (K - 1, 2, 0):
            hist = prev.to(dev)
            got, _ = ops.sampler_step(out_c, off, y_d, z_d, torch.full((B,), k, device=dev), plan, B, max_v, True,
                                      y0_prev=hist, threshold=0.9)
            want, want_y0, s = prediction_ref.sampler_step(betas, tau, "dpmpp2m", 0.0, prediction, k, y64, comp, prev64, z64,
                                                           q=0.9)
            errs = (rel(got, want), rel(hist, want_y0))
            scales.append(s)
            print(f"{prediction} threshold 0.9 dpmpp2m k {k}: s {s}  y_new rel {errs[0]:.2e}  y0 rel {errs[1]:.2e}")
            assert max(errs) <= KERNEL_RTOL
        assert max(float(s.max()) for s in scales) > 1.0               # (the threshold does something)
    finally:
        vf.set_prediction("eps")


# ---- 5. model level ----------------------------------------------------------------------------------------------------------
def test_forward_under_v_is_compose_loss_on_the_built_target(dev):
    from view_fusion_amd import ops
    B = 3
    batch, inj = _batch(dev, B, VC), _inject(dev, B)
    vf = _model(dev)
    vf.set_prediction("v")
    loss = vf(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"], **inj)
    loss.backward()
    assert all(torch.isfinite(p.grad).all() for p in vf.parameters())
    with torch.no_grad():
        level = ops.gather_level(vf.gammas, inj["t"], inj["u"].reshape(-1).contiguous())
        off, S, _ = ops.view_offsets(batch["view_count"], dev)
        x, level_s, angle_s = ops.stack_views(batch["y_cond"], batch["y_0"], inj["noise"], level, batch["angle"], off, S)
        out = vf.denoise_fn(x, angle_s, level_s)
        lv = level.reshape(B, 1, 1, 1)
        target = lv.sqrt() * inj["noise"] - (1 - lv).sqrt() * batch["y_0"]           # fp32, built explicitly
        want, sl = ops.compose_loss(out, target, off, B, True, level)
    loss = loss.detach()
    print(f"forward under v {float(loss):.9g}  compose_loss on the fp32 target {float(want):.9g}")
    assert close(float(loss), float(want)) and close(vf.last_sample_loss.cpu().numpy(), sl.cpu().numpy())
    eps = _model(dev)
    loss_e = eps(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"], **inj)
    assert not close(float(loss), float(loss_e.detach()))                       # (another objective than eps)


@pytest.fixture(scope="module")
def case(dev):
    """Inputs, injected draws and the oracle UNet, made once and left unchanged."""
    from oracle import unet_ref, view_fusion_ref as vfr
    g = torch.Generator().manual_seed(910)
    HW = TINY["image_size"]
    c = dict(y_cond=torch.rand(3, 3, 3, HW, HW, generator=g),
             angle=2 * np.pi / 24 * torch.randint(0, 24, (3, 1), generator=g).float(),
             y_T=torch.randn(3, 3, HW, HW, generator=g), z_seq=torch.randn(T, 3, 3, HW, HW, generator=g),
             vc=torch.tensor(VC))
    sd = {k: v.detach().cpu().clone() for k, v in _model(dev).denoise_fn.state_dict().items()}
    c["unet"] = lambda x, a, l: unet_ref.unet_forward(sd, TINY, x, a, l)
    c["compose"] = vfr.compose
    c["gpu"] = {k: c[k].to(dev) for k in ("y_cond", "angle", "y_T", "z_seq")}
    return c


def _ref_chain(case, sched_kw, prediction, tau, solver, z_seq, y_T=None):
    from oracle import view_fusion_ref as vfr
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**sched_kw)                     # (float64; vfr has no zero-terminal variant)
    if sched_kw.get("zero_terminal_snr"):
        with np.errstate(divide="ignore"):                             # g^-1/2 at gamma = 0: the pair is substituted
            bufs = vfr.schedule_buffers(betas)
    else:
        bufs = vfr.schedule_buffers(vfr.beta_schedule(**sched_kw))
    with torch.no_grad(), np.errstate(divide="ignore"):                 # (lambda = -inf at gamma = 0)
        return prediction_ref.chain(case["unet"], case["compose"], np.asarray(betas, dtype=np.float64), bufs, prediction,
                                    case["y_cond"], case["vc"], case["angle"], case["y_T"] if y_T is None else y_T, z_seq, tau=tau,
                                    solver=solver)


@pytest.mark.parametrize("kind", ["dpmpp2m-4", "ancestral"])
def test_generate_under_v_against_the_float64_chain(dev, case, kind):
    from view_fusion_amd import schedule
    vf = _model(dev)
    vf.set_prediction("v")
    g = case["gpu"]
    if kind == "ancestral":
        y, ret, _, _, samples = vf.generate(g["y_cond"], case["vc"], g["angle"], y_t=g["y_T"], z_seq=g["z_seq"],
                                            sample_num=T - 1)
        states = _ref_chain(case, SCHED, "v", None, "ddim", case["z_seq"])
        keep = [i for i, t in enumerate(reversed(range(T))) if t % max(1, T // (T - 1)) == 0]
    else:
        K = 4                                                           # seeded: y_T is the counter-based draw
        y, ret, _, _, samples = vf.generate(g["y_cond"], case["vc"], g["angle"], seed=77, sample_ids=[5, 9, 2 ** 34],
                                            sample_steps=K, solver="dpmpp2m")
        assert not torch.equal(ret[:, 0], g["y_T"])
        states = _ref_chain(case, SCHED, "v", schedule.sample_timesteps(T, K), "dpmpp2m", None, y_T=ret[:, 0].cpu())
        keep = list(range(K))
    assert ret.shape[1] == 1 + len(keep)
    err = float((ret[:, 1:].cpu() - states[keep].transpose(0, 1)).abs().max())
    print(f"generate under v, {kind}: chain max-abs {err:.3e} against the float64 chain")
    assert torch.equal(y, samples) and err <= CHAIN_TOL
    # the eps reading of the same weights is another sample
    vf.set_prediction("eps")
    kw = dict(z_seq=g["z_seq"]) if kind == "ancestral" else dict(sample_steps=4, solver="dpmpp2m")
    other = vf.generate(g["y_cond"], case["vc"], g["angle"], y_t=ret[:, 0].contiguous(), **kw)[4]
    assert float((other - samples).abs().max()) > 10 * CHAIN_TOL


@pytest.mark.parametrize("prediction", PREDS)
def test_generate_on_a_zero_terminal_schedule(dev, case, prediction):
    from view_fusion_amd import schedule
    zsched = dict(SCHED, zero_terminal_snr=True)
    vf = _model(dev, zsched)
    assert float(vf.gammas[-1]) == 0.0
    g = case["gpu"]
    with pytest.raises(ValueError, match="zero"):
        vf.generate(g["y_cond"], case["vc"], g["angle"], y_t=g["y_T"], sample_steps=3)
    vf.set_prediction(prediction)
    for kw, tau, solver, z in ((dict(sample_steps=3, solver="dpmpp2m"), schedule.sample_timesteps(T, 3), "dpmpp2m", None),
                               (dict(z_seq=g["z_seq"], sample_num=T - 1), None, "ddim", case["z_seq"])):
        y, ret, logits, weights, samples = vf.generate(g["y_cond"], case["vc"], g["angle"], y_t=g["y_T"], **kw)
        assert all(torch.isfinite(x).all() for x in (y, ret, logits, weights, samples))
        states = _ref_chain(case, zsched, prediction, tau, solver, z)
        err = float((samples.cpu() - states[-1]).abs().max())
        print(f"zero terminal SNR, {prediction}, {'ancestral' if tau is None else 'dpmpp2m K = 3'}: finite; final sample "
              f"max-abs {err:.3e} against the float64 chain")
        assert err <= CHAIN_TOL


# ---- 6. Trainer --------------------------------------------------------------------------------------------------------------
TB, TVC, TK, SEED = 4, [1, 3, 2, 2], 4, 11


def _trainer(dev, graph, **kw):
    from view_fusion_amd import train
    vf = _model(dev)
    vf.set_prediction("v")
    vf.set_loss(weighting="min_snr", snr_gamma=1.0)
    vf.set_level_sampler("fixed", bins=TK, probs=[1.0, 2.0, 3.0, 2.0])
    tr = train.Trainer(vf, lr_warmup=1, graph=graph, seed=SEED, loss_bins=TK, **kw)
    tr.it = 0
    return vf, tr


def _steps(dev, vf, tr, n, first=0):
    out = []
    for s in range(first, first + n):
        loss = tr.step(_batch(dev, TB, TVC, s)).clone()
        out.append((loss, vf.last_sample_loss.clone(), vf.last_level.clone()))
    return out


def _same(a, b):
    return all(torch.equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def test_trainer_graph_replay_equals_eager_and_follows_set_prediction(dev):
    (vf_e, tr_e), (vf_g, tr_g), (vf_v, tr_v) = _trainer(dev, False), _trainer(dev, True), _trainer(dev, False)
    re_, rg, rv = _steps(dev, vf_e, tr_e, 3), _steps(dev, vf_g, tr_g, 3), _steps(dev, vf_v, tr_v, 3)
    assert tr_e.graph_steps == 0 and tr_g.graph_steps == 1 and tr_g.mode == "graph"
    assert _same(re_, rg) and _same(re_, rv)
    assert all(torch.equal(p, q) for p, q in zip(vf_e.parameters(), vf_g.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(vf_e.loss_hist, vf_g.loss_hist))
    assert int(vf_g.loss_hist[1].sum()) == 3 * TB
    # the returned loss is importance weight x native weight x native per-sample loss
    w = prediction_ref.weights(rg[2][2].cpu().numpy(), "v", "min_snr", 1.0)
    iw = vf_g.last_importance_weight.cpu().numpy().astype(np.float64)
    assert close(float(rg[2][0]), float((iw * w * rg[2][1].cpu().numpy()).mean()))
    # set_prediction after the capture: the captured step is dropped, the next step runs the new objective
    for m in (vf_e, vf_g):
        m.set_prediction("x0")
    ne, ng, nv = _steps(dev, vf_e, tr_e, 1, first=3), _steps(dev, vf_g, tr_g, 1, first=3), _steps(dev, vf_v, tr_v, 1, first=3)
    print(f"step 4: x0 after the switch {float(ng[0][0]):.9g} (eager twin {float(ne[0][0]):.9g}); v would give {float(nv[0][0]):.9g}")
    assert tr_g.graph_steps == 1                                        # step 4 ran eagerly: the graph was dropped
    assert _same(ne, ng) and torch.equal(ng[0][2], nv[0][2])            # the same draws ...
    assert not close(float(ng[0][0]), float(nv[0][0]))                  # ... another loss
    assert not close(ng[0][1].cpu().numpy(), nv[0][1].cpu().numpy())


def test_trainer_accum_steps_under_v(dev):
    (vf_e, tr_e), (vf_g, tr_g) = _trainer(dev, False, accum_steps=2), _trainer(dev, True, accum_steps=2)
    re_, rg = _steps(dev, vf_e, tr_e, 3), _steps(dev, vf_g, tr_g, 3)
    assert tr_g.graph_steps >= 1 and _same(re_, rg)
    assert all(torch.equal(p, q) for p, q in zip(vf_e.parameters(), vf_g.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(vf_e.loss_hist, vf_g.loss_hist))
    assert int(vf_g.loss_hist[1].sum()) == 3 * TB and vf_g.last_sample_loss.numel() == TB // 2
