"""A learned variance on the GPU (ViewFusion.set_learned_variance, ops.compose_loss(vlb=), ops.sampler_step(variance=);
the LV instantiations of the loss family -- compose_loss_fwd_kernel / _bwd_kernel<PEN, PRED, true> and the vlb operands of
compose_loss_finish_kernel -- and sampler_step_lv_kernel<CFG, RNG> of csrc/diffusion.hip; definition
at the head of that file, arithmetic in csrc/vlb.h) against the float64 restatement tests/vlb_ref.py.

  1. the hybrid loss against float64: softmax and mean; eps, v and x0; mse and huber (+ min_snr); t in {1, 7, T-1} on the
     T = 20 linear schedule, at the shapes of test_gpu_loss_options.py for the reasons it gives (8x8: fewer float4s than one
     workgroup; 12x20: n4 % 256 != 0; 128x192 at B = 1: the grid-stride loop and all 64 partials).  Channels 0..5 as
     test_gpu_prediction.py builds them (|d| >= 0.01), channels 6..8 uniform in [-1.2, 1.2].  The L_simple quantities keep
     the loss-options tolerances (close(): 1e-6 |b| + 1e-7; d unet_out channels 0..2 max-relative 1e-5).  The vlb quantities
     and channels 3..8 get no number fixed in advance -- exp(-lp) amplifies the fp32 rounding of lp at small t: the SAME
     restatement evaluated in numpy float32 on the same inputs measures its own distance from float64, and the device may
     be 4 x as far (summation order, expf against numpy's exp), per quantity and per sample, floored at the loss-options
     tolerances.  The gradient is compared per sample (max-abs difference over the sample's max-abs): the t = 1 sample's
     is orders of magnitude larger than the others'.  The float64 gradient is autograd's with r detached.  No element is
     excluded.
  2. the stop-gradient: channels 0..2 of d unet_out equal those of ops.compose_loss without vlb= bit for bit; float64
     autograd WITHOUT the detach differs from it by far more than the tolerance.
  3. the tail against the restatement: all four instantiations at 8x8 and 12x20, k in {0, 2, 4} of a K = 5 chain, within
     the sampler tests' kernel tolerance (rel 2e-5).  Bit for bit: at k = 0 no noise is read or drawn; CFG at g = 1 is the
     unguided kernel; the RNG flavour is the loaded-z flavour fed the device's own normals of the same counters (and
     within rng_ref's bound of the float64 normals -- rng_ref's are another evaluation of Box-Muller, so not bit for bit);
     with hi == lo == log beta~ and o = 0 (v = 1/2: lp is the table value exactly) the step is ops.sampler_step's eta = 1
     step on a sigma table holding the device's own expf(0.5 log beta~) -- read back from the kernel through y = out = 0,
     z = 1 and checked against float64 within 2 ulp -- since a float64 sqrt(beta~) rounded once need not be that expf.
  4. model level, TINY with out_channel=9: forward() is the op on explicitly stacked inputs; generate() at
     sample_steps=None and K = 4, eta = 1 against the float64 chain through the oracle UNet (max-abs 1e-3, the sampler
     tests' chain tolerance); dpmpp2m / eta = 0 run the existing kernels; three logit channels; guidance is finite.
  5. Trainer: graph replay == eager bit for bit over three steps; accum_steps = 2 against the undivided batch within
     test_gpu_grad_accum.py's bound (4 e + 1e-7 max|g|, e the undivided batch's distance from the float64 oracle);
     set_learned_variance(None) after a capture drops the graph; a 6-channel model that touched the setter and turned it
     off runs the launch list and the bits of one that never did.
  6. the refusals that need a device.
Figures are printed before the assertions (run with -s); profiles/learned_variance.md records them."""
import numpy as np
import pytest
import torch

import loss_ref
import rng_ref
import vlb_ref
from conftest import TINY

pytestmark = pytest.mark.gpu
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
T = SCHED["num_timesteps"]
NINE = dict(TINY, out_channel=9)
SHAPES = {"8x8": ((8, 8), (1, 3, 2)), "12x20": ((12, 20), (1, 3, 2)), "128x192": ((128, 192), (2,))}
TS = {"8x8": [(1, 7, T - 1)], "12x20": [(1, 7, T - 1)], "128x192": [(1,), (7,), (T - 1,)]}
PREDS = ("eps", "v", "x0")
PEN_CASES = [("mse", None, 0.0, 0.0), ("huber", "min_snr", 5.0, 0.0)]
DELTA, LAM, GLOSS = 0.7, 0.3, 1.7
KERNEL_RTOL, CHAIN_TOL = 2e-5, 1e-3          # test_gpu_sampler_steps.py: one kernel (max|a-b| / max|b|), a chain (max-abs)
VC = [1, 3, 2]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tabs():
    """The fp32 table values the device reads, on the host: c1, hi, lo, gammas (T,) and the float64 betas."""
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**SCHED)
    bufs = schedule.schedule_tensors(betas, "cpu")
    hi, lo = (x.astype(np.float32) for x in schedule.variance_tables(betas))
    return dict(betas=np.asarray(betas, dtype=np.float64), c1=bufs["posterior_mean_coef1"].numpy(), hi=hi, lo=lo,
                gammas=bufs["gammas"].numpy())


def rel(a, b):
    a, b = (torch.as_tensor(x).detach().double().cpu().numpy() for x in (a, b))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def close(a, b):
    """test_gpu_loss_options.py's loss tolerance, element by element."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) < 1e-6 * np.abs(b) + 1e-7))


_INPUTS = {}


def _inputs(tabs, shape, weighting, prediction, ts):
    """Fixed-seed unet_out (9 channels) / noise / y_0 / level of one case, built once and left unchanged: channels 0..5,
    the wanted target noise_hat - sign (0.01 + |N|), the noise and the solved y_0 as test_gpu_prediction.py builds them
    (the same generator), then channels 6..8 uniform in [-1.2, 1.2]; level[b] = the middle of [gammas[t], gammas[t-1]]."""
    key = (shape, weighting, prediction, ts)
    if key not in _INPUTS:
        (H, W), vc = SHAPES[shape]
        g = torch.Generator().manual_seed(3)
        out6 = (torch.randn(sum(vc), 6, H, W, generator=g) * 2).numpy()
        nh, _ = loss_ref.compose(out6, vc, weighting)
        mag = 0.01 + torch.randn(len(vc), 3, H, W, generator=g).abs().double().numpy()
        sign = np.where(torch.rand(len(vc), 3, H, W, generator=g).numpy() < 0.5, -1.0, 1.0)
        want = nh - sign * mag
        noise = torch.randn(len(vc), 3, H, W, generator=g).numpy()
        var = (torch.rand(sum(vc), 3, H, W, generator=g) * 2.4 - 1.2).numpy()
        gam = tabs["gammas"].astype(np.float64)
        level = np.array([0.5 * (gam[t] + gam[t - 1]) for t in ts], dtype=np.float32)
        lv = level.astype(np.float64).reshape(-1, 1, 1, 1)
        if prediction == "eps":
            noise, y_0 = want.astype(np.float32), None                 # the target, ready-made
        elif prediction == "v":
            y_0 = ((np.sqrt(lv) * noise.astype(np.float64) - want) / np.sqrt(1.0 - lv)).astype(np.float32)
        else:
            y_0 = want.astype(np.float32)
        _INPUTS[key] = (np.concatenate([out6, var], axis=1), noise, y_0, level, vc)
    return _INPUTS[key]


def _run_op(dev, tabs, out, noise, y_0, level, vc, ts, weighting, prediction, penalty, kind, a, b, lam=LAM):
    from view_fusion_amd import ops
    off, S, _ = ops.view_offsets(list(vc), dev)
    og = torch.from_numpy(out).to(dev).requires_grad_(True)
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)             # noqa: E731
    pred = {} if prediction == "eps" else dict(prediction=prediction, y_0=dv(y_0))
    vlb = None if lam is None else (torch.tensor(ts, device=dev), dv(tabs["c1"]), dv(tabs["hi"]), dv(tabs["lo"]), lam)
    res = ops.compose_loss(og, dv(noise), off, len(vc), weighting, dv(level), penalty, DELTA, kind, a, b, vlb=vlb, **pred)
    loss, sl = res[0], res[1]
    assert all(not x.requires_grad for x in res[1:]) and loss.requires_grad
    (loss * GLOSS).backward()
    sv = res[2].cpu().numpy() if lam is not None else None
    return float(loss.detach()), sl.cpu().numpy(), sv, og.grad.cpu().numpy()


def _reference(tabs, out, noise, y_0, level, vc, ts, weighting, prediction, penalty, kind, a, b):
    """float64: the numpy restatement, its gradient from autograd with r detached; float32: the same restatement."""
    args = (noise, y_0, vc, weighting, level, ts, tabs["c1"], tabs["hi"], tabs["lo"], LAM, prediction, penalty, DELTA,
            kind, a, b)
    r64 = vlb_ref.hybrid(out, *args, gloss=GLOSS)
    r32 = vlb_ref.hybrid(out, *args, gloss=GLOSS, dtype=np.float32)
    o = torch.tensor(out, dtype=torch.float64, requires_grad=True)
    loss, _, _ = vlb_ref.hybrid_torch(o, *args)
    (loss * GLOSS).backward()
    assert abs(float(loss.detach()) - r64["loss"]) <= 1e-11 * abs(r64["loss"])
    return r64, r32, o.grad.numpy()


def _rel_rows(a, b, rows, ch):
    a, b = a[rows][:, ch].astype(np.float64), np.asarray(b[rows][:, ch], dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- 1. the op against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_hybrid_loss_against_float64(dev, tabs, shape, weighting):
    failures, worst = [], {}
    for ts in TS[shape]:
        for prediction in PREDS:
            out, noise, y_0, level, vc = _inputs(tabs, shape, weighting, prediction, ts)
            n4 = 3 * out.shape[2] * out.shape[3] // 4
            assert (n4 < 256) if shape == "8x8" else (n4 > 64 * 256) if shape == "128x192" else (n4 % 256 != 0)
            off = loss_ref.offsets(vc)
            for penalty, kind, a, b in PEN_CASES:
                case = (ts, prediction, penalty)
                r64, r32, g64 = _reference(tabs, out, noise, y_0, level, vc, ts, weighting, prediction, penalty, kind, a, b)
                assert np.abs(r64["d"]).min() >= 1e-3                  # the residual: no element near a kink, none excluded
                loss, sl, sv, dout = _run_op(dev, tabs, out, noise, y_0, level, vc, ts, weighting, prediction, penalty,
                                             kind, a, b)
                assert np.isfinite(dout).all()                         # all nine channels written
                e32 = abs(float(r32["loss"]) - r64["loss"])
                e = abs(loss - r64["loss"])
                ok = e <= max(4.0 * e32, 1e-6 * abs(r64["loss"]) + 1e-7) and close(sl, r64["sample_loss"])
                print(f"{shape} softmax={weighting} t {ts} {prediction:3s} {penalty:5s}: loss {loss:.9g} (f64 "
                      f"{r64['loss']:.12g}) |diff| {e:.2e}  fp32 restatement {e32:.2e};  sample_loss rel "
                      f"{float((np.abs(sl - r64['sample_loss']) / np.abs(r64['sample_loss'])).max()):.2e}")
                for i, t in enumerate(ts):
                    rows = slice(int(off[i]), int(off[i + 1]))
                    ref_v = r64["sample_vlb"][i]
                    ev32 = abs(float(r32["sample_vlb"][i]) - ref_v) / abs(ref_v)
                    ev = abs(float(sv[i]) - ref_v) / abs(ref_v)
                    ok = ok and ev <= max(4.0 * ev32, 1e-6 + 1e-7 / abs(ref_v))
                    ed = [_rel_rows(dout, g64, rows, ch) for ch in (slice(0, 3), slice(3, 6), slice(6, 9))]
                    ed32 = [_rel_rows(r32["dout"], g64, rows, ch) for ch in (slice(0, 3), slice(3, 6), slice(6, 9))]
                    ok = ok and ed[0] < 1e-5 and all(x <= max(4.0 * y, 1e-5) for x, y in zip(ed[1:], ed32[1:]))
                    for name, x, y in (("vlb", ev, ev32), ("d3..5", ed[1], ed32[1]), ("d6..8", ed[2], ed32[2])):
                        w = worst.setdefault((t, name), [0.0, 0.0])
                        w[0], w[1] = max(w[0], x), max(w[1], y)
                    print(f"    sample {i} t {t:2d}: vlb {float(sv[i]):.7g} bits rel {ev:.2e} (fp32 restatement {ev32:.2e})  "
                          f"dout rel 0..2 {ed[0]:.2e}  3..5 {ed[1]:.2e} ({ed32[1]:.2e})  6..8 {ed[2]:.2e} ({ed32[2]:.2e})  "
                          f"max|g| {np.abs(g64[rows]).max():.3e}")
                    if off[i + 1] - off[i] == 1 or not weighting:
                        assert np.all(dout[rows, 3:6] == 0), case          # one view / the mean: zero logit gradient
                if not ok:
                    failures.append(case)
    for (t, name), (x, y) in sorted(worst.items()):
        print(f"{shape} softmax={weighting} worst at t {t:2d} {name:6s}: device {x:.2e}  fp32 restatement {y:.2e}")
    assert not failures, failures


def test_launches_histogram_and_determinism(dev, tabs):
    """Two launches forward and one backward; the histogram receives the unweighted L_simple per-sample loss; two runs
    give the same bits."""
    from view_fusion_amd import ops
    ts = TS["12x20"][0]
    out, noise, y_0, level, vc = _inputs(tabs, "12x20", True, "v", ts)
    off, S, _ = ops.view_offsets(list(vc), dev)
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)             # noqa: E731
    Kb = 5
    hist = (torch.zeros(Kb, device=dev), torch.zeros(Kb, device=dev, dtype=torch.int32))
    runs = []
    for rep in range(2):
        og = dv(out).requires_grad_(True)
        ops.st.KERNEL_LOG = []
        try:
            loss, sl, w, sv = ops.compose_loss(og, dv(noise), off, 3, True, dv(level), "huber", DELTA, "min_snr", 5.0, 0.0,
                                               hist=hist if rep == 0 else None, want_weight=True, prediction="v",
                                               y_0=dv(y_0), vlb=(torch.tensor(ts, device=dev), dv(tabs["c1"]),
                                                                 dv(tabs["hi"]), dv(tabs["lo"]), LAM))
            loss.backward()
            names = [r[5] for r in ops.st.KERNEL_LOG]
        finally:
            ops.st.KERNEL_LOG = None
        assert names == ["vf_compose_loss_lv_fwd", "vf_compose_loss_lv_bwd"]
        runs.append((loss.detach().clone(), sl.clone(), sv.clone(), og.grad.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    s, c = loss_ref.histogram(level, runs[0][1].cpu().numpy(), Kb)
    assert np.array_equal(hist[1].cpu().numpy(), c) and c.sum() == 3
    assert np.all(np.abs(hist[0].cpu().numpy() - s) <= 4 * 2.0 ** -24 * np.abs(s))
    assert close(w.cpu().numpy(), ops.loss_weights_pred_host(level, "v", "min_snr", 5.0, 0.0).numpy())


# ---- 2. the stop-gradient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("prediction", PREDS)
def test_the_mean_gets_no_gradient_from_the_vlb_term(dev, tabs, prediction, weighting):
    ts = TS["12x20"][0]
    out, noise, y_0, level, vc = _inputs(tabs, "12x20", weighting, prediction, ts)
    for penalty, kind, a, b in PEN_CASES:
        _, sl, _, dout = _run_op(dev, tabs, out, noise, y_0, level, vc, ts, weighting, prediction, penalty, kind, a, b)
        _, sl0, _, dout0 = _run_op(dev, tabs, out, noise, y_0, level, vc, ts, weighting, prediction, penalty, kind, a, b,
                                   lam=None)
        assert np.array_equal(dout[:, 0:3], dout0[:, 0:3])            # L_simple's alone, to the bit
        assert close(sl, sl0)                                          # (its partial sums are another kernel's)
        assert np.abs(dout[:, 6:9]).min() > 0                          # (lambda > 0: the variance channels do get one)
        args = (noise, y_0, vc, weighting, level, ts, tabs["c1"], tabs["hi"], tabs["lo"], LAM, prediction, penalty, DELTA,
                kind, a, b)
        o = torch.tensor(out, dtype=torch.float64, requires_grad=True)
        (vlb_ref.hybrid_torch(o, *args, detach=False)[0] * GLOSS).backward()
        flowing = o.grad.numpy()
        off = loss_ref.offsets(vc)
        for i in range(len(vc)):
            rows = slice(int(off[i]), int(off[i + 1]))
            d = _rel_rows(dout, flowing, rows, slice(0, 3))
            print(f"{prediction} softmax={weighting} {penalty} sample {i}: device against a FLOWING mean, channels 0..2 rel {d:.2e}")
            assert d > 1e-3                                            # far more than the 1e-5 the detached one is held to


# ---- 3. the tail ---------------------------------------------------------------------------------------------------------
def _model(dev, cfg=NINE, sched=SCHED):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**cfg)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": dict(sched)}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


@pytest.fixture(scope="module")
def vf(dev):
    m = _model(dev)
    m.set_learned_variance()
    return m


def _tail_inputs(H, W):
    g = torch.Generator().manual_seed(23 + H)
    out = torch.randn(sum(VC) + 3, 9, H, W, generator=g) * 2            # the null rows last
    out[:, 6:9] = torch.rand(sum(VC) + 3, 3, H, W, generator=g) * 2.4 - 1.2
    y, z = (torch.randn(3, 3, H, W, generator=g) for _ in range(2))
    return out, y, z


@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("H,W", [(8, 8), (12, 20)])
def test_tail_against_the_restatement(vf, dev, tabs, H, W, weighting):
    from view_fusion_amd import ops, schedule
    B, K, S = 3, 5, sum(VC)
    seed, ids = 0x5EED, [3, 2 ** 33 + 5, 11]
    tau = schedule.sample_timesteps(T, K)
    plan = vf._lv_plan(tau.tolist(), dev)
    var = (plan["hi"], plan["lo"])
    hi32, lo32 = plan["hi"].cpu().numpy(), plan["lo"].cpu().numpy()
    out, y, z = _tail_inputs(H, W)
    off, _, max_v = ops.view_offsets(VC, dev)
    nh, ob, _ = vlb_ref.compose9(out[:S].numpy(), VC, weighting)
    gsc = np.array([0.0, 1.0, 2.5])
    nh_g = gsc.reshape(3, 1, 1, 1) * nh + (1.0 - gsc.reshape(3, 1, 1, 1)) * out[S:, 0:3].double().numpy()
    out_d, y_d, z_d = out.to(dev), y.to(dev), z.to(dev)
    gs = ops.guidance_scales(dev, B, gsc.tolist())
    ids_d = ops.sample_ids(dev, B, ids)
    worst = 0.0
    for k in (0, 2, K - 1):
        kk = torch.full((B,), k, device=dev)
        z_rng = rng_ref.normal(seed, ids, rng_ref.KIND_STEP_NOISE, int(tau[k]), 3 * H * W).reshape(B, 3, H, W)
        for cfg in (False, True):
            src = dict(guidance=gs, S=S) if cfg else {}
            o_in = out_d if cfg else out_d[:S].contiguous()
            comp = nh_g if cfg else nh
            for rng in (False, True):
                noise = dict(seed=seed, ids=ids_d) if rng else {}
                hist = torch.full((B, 3, H, W), float("nan"), device=dev)
                got, wts, lp = ops.sampler_step(o_in, off, y_d, None if rng else z_d, kk, plan, B, max_v, weighting,
                                                y0_prev=hist, variance=var, want_logvar=True, **src, **noise)
                want, want_y0, want_lp = vlb_ref.sampler_step(tabs["betas"], tau, "eps", k, y.double().numpy(), comp, ob,
                                                              z_rng if rng else z.double().numpy(), hi32, lo32)
                errs = (rel(got, want), rel(hist, want_y0), rel(lp, want_lp))
                worst = max(worst, *errs)
                print(f"{H}x{W} weighting {weighting} k {k} cfg {cfg} rng {rng}: y_new rel {errs[0]:.2e}  y0 rel "
                      f"{errs[1]:.2e}  lp rel {errs[2]:.2e}")
                assert torch.isfinite(got).all() and max(errs) <= KERNEL_RTOL
                assert (wts is not None) == weighting
                if weighting:                                           # the weights are the existing tail's
                    plain = ops.sampler_step(o_in, off, y_d, None, kk, plan, B, max_v, True, **src)[1]
                    assert torch.equal(wts, plain)
    print(f"{H}x{W} weighting {weighting}: worst rel against the float64 restatement {worst:.2e}")


@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("H,W", [(8, 8), (12, 20)])
def test_tail_bit_for_bit(vf, dev, H, W, weighting):
    from view_fusion_amd import ops, schedule
    B, K, S = 3, 5, sum(VC)
    seed, ids = 77, [40, 2 ** 35, 43]
    tau = schedule.sample_timesteps(T, K)
    plan = vf._lv_plan(tau.tolist(), dev)
    var = (plan["hi"], plan["lo"])
    out, y, z = _tail_inputs(H, W)
    off, _, max_v = ops.view_offsets(VC, dev)
    out_d, y_d, z_d = out.to(dev), y.to(dev), z.to(dev)
    out_c = out_d[:S].contiguous()
    ids_d = ops.sample_ids(dev, B, ids)
    ones = ops.guidance_scales(dev, B, 1.0)
    step = lambda o, zz, k, **kw: ops.sampler_step(o, off, y_d, zz, torch.full((B,), k, device=dev), plan, B, max_v,  # noqa: E731
                                                   weighting, variance=var, **kw)[0]
    # k = 0: no noise is read (a NaN buffer leaves no trace) or drawn
    base = step(out_c, None, 0)
    assert torch.equal(step(out_c, torch.full_like(z_d, float("nan")), 0), base)
    assert torch.equal(step(out_c, None, 0, seed=seed, ids=ids_d), base) and torch.isfinite(base).all()
    for k in (0, 2, K - 1):
        plain = step(out_c, z_d, k)
        if k:
            assert not torch.equal(plain, step(out_c, None, k))        # (the noise does arrive)
        # CFG at g = 1 is the unguided kernel
        assert torch.equal(step(out_d, z_d, k, guidance=ones, S=S), plain)
        # the RNG flavour: the loaded-z flavour fed the device's own normals of (seed, id, tau[k]) ...
        zz = torch.stack([ops.randn_ids(seed, ops.sample_ids(dev, 1, [i]), 3, int(tau[k]), (3, H, W))[0] for i in ids])
        drawn = step(out_c, None, k, seed=seed, ids=ids_d)
        assert torch.equal(drawn, step(out_c, zz, k))
        assert torch.equal(step(out_d, None, k, seed=seed, ids=ids_d, guidance=ones, S=S), drawn)
        # ... which are rng_ref's within its bound (scaled by the largest noise scale, exp(0.5 hi[k]) at v <= 1.1)
        r64, e, bound = rng_ref.bound(seed, ids, rng_ref.KIND_STEP_NOISE, int(tau[k]), 3 * H * W)
        assert float(np.abs(zz.double().cpu().numpy().reshape(B, -1) - r64).max()) <= bound
    # hi == lo == log beta~ and o = 0: ops.sampler_step's eta = 1 step on the device's own expf(0.5 log beta~)
    flat = (plan["lo"], plan["lo"])
    zero9 = torch.zeros(S, 9, H, W, device=dev)
    sd = torch.stack([ops.sampler_step(zero9, off, torch.zeros_like(y_d), torch.ones_like(z_d), torch.full((B,), k, device=dev),
                                       plan, B, max_v, weighting, variance=flat)[0].flatten()[0] for k in range(K)])
    sd64 = np.exp(0.5 * plan["lo"].double().cpu().numpy())
    print(f"{H}x{W} weighting {weighting}: expf(0.5 lo) {sd.cpu().numpy()}  float64 {sd64}  table sigma {plan['sigma'].cpu().numpy()}")
    assert float(sd[0]) == 0.0                                          # (k = 0: no noise at all)
    assert np.all(np.abs(sd.double().cpu().numpy()[1:] - sd64[1:]) <= 2.0 ** -22 * sd64[1:])
    assert np.all(np.abs(sd64[1:] - plan["sigma"].double().cpu().numpy()[1:]) <= 1e-6 * sd64[1:])
    o0 = out_c.clone()
    o0[:, 6:9] = 0
    plan_sd = dict(plan, sigma=sd.contiguous())
    for k in range(K):
        kk = torch.full((B,), k, device=dev)
        h1, h2 = torch.empty_like(y_d), torch.empty_like(y_d)
        a = ops.sampler_step(o0, off, y_d, z_d, kk, plan, B, max_v, weighting, y0_prev=h1, variance=flat)[0]
        b = ops.sampler_step(o0, off, y_d, z_d, kk, plan_sd, B, max_v, weighting, y0_prev=h2)[0]
        assert torch.equal(a, b) and torch.equal(h1, h2), k


# ---- 4. model level --------------------------------------------------------------------------------------------------------
def _batch(dev, B, vc, s=0):
    from view_fusion_amd import train
    return dict(train.synthetic_batch(B, 3, 16, dev, seed=40 + s), view_count=torch.tensor(vc))


def _inject(dev, B):
    g = torch.Generator().manual_seed(1)
    return dict(t=torch.tensor([15, 1, 9])[:B].to(dev), u=torch.rand(B, 1, generator=g).to(dev),
                noise=torch.randn(B, 3, 16, 16, generator=g).to(dev))


@pytest.mark.parametrize("prediction", ["eps", "v"])
def test_forward_is_the_op_on_stacked_inputs(dev, prediction):
    from view_fusion_amd import ops
    B = 3
    batch, inj = _batch(dev, B, VC), _inject(dev, B)
    m = _model(dev)
    m.set_learned_variance(LAM)
    m.set_prediction(prediction)
    loss = m(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"], **inj)
    loss.backward()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    head = [p for n, p in m.named_parameters() if "final_conv" in n and p.dim() == 4][0]
    assert head.shape[0] == 9 and float(head.grad[6:9].abs().max()) > 0     # the variance rows of the head get a gradient
    with torch.no_grad():
        level = ops.gather_level(m.gammas, inj["t"], inj["u"].reshape(-1).contiguous())
        off, S, _ = ops.view_offsets(batch["view_count"], dev)
        x, level_s, angle_s = ops.stack_views(batch["y_cond"], batch["y_0"], inj["noise"], level, batch["angle"], off, S)
        out = m.denoise_fn(x, angle_s, level_s)
        assert out.shape[1] == 9
        pred = {} if prediction == "eps" else dict(prediction="v", y_0=batch["y_0"])
        want, sl, sv = ops.compose_loss(out, inj["noise"], off, B, True, level, vlb=(inj["t"], *m._lv_tables(), LAM), **pred)
        plain, _ = ops.compose_loss(out, inj["noise"], off, B, True, level, **pred)
    print(f"forward ({prediction}) {float(loss.detach()):.9g}  the op {float(want):.9g}  L_simple alone {float(plain):.9g}  "
          f"vlb {m.last_sample_vlb.cpu().numpy()} bits")
    assert close(float(loss.detach()), float(want)) and close(m.last_sample_loss.cpu().numpy(), sl.cpu().numpy())
    assert close(m.last_sample_vlb.cpu().numpy(), sv.cpu().numpy()) and not m.last_sample_vlb.requires_grad
    assert close(float(want), float(plain) + LAM * float(sv.double().mean()))


@pytest.fixture(scope="module")
def case(dev):
    """Inputs, injected draws and the oracle UNet on the nine-channel weights, made once and left unchanged."""
    from oracle import unet_ref
    g = torch.Generator().manual_seed(910)
    HW = TINY["image_size"]
    c = dict(y_cond=torch.rand(3, 3, 3, HW, HW, generator=g),
             angle=2 * np.pi / 24 * torch.randint(0, 24, (3, 1), generator=g).float(),
             y_T=torch.randn(3, 3, HW, HW, generator=g), z_seq=torch.randn(T, 3, 3, HW, HW, generator=g),
             vc=torch.tensor(VC))
    sd = {k: v.detach().cpu().clone() for k, v in _model(dev).denoise_fn.state_dict().items()}
    c["unet"] = lambda x, a, l: unet_ref.unet_forward(sd, NINE, x, a, l)
    c["gpu"] = {k: c[k].to(dev) for k in ("y_cond", "angle", "y_T", "z_seq")}
    return c


@pytest.mark.parametrize("kind", ["full", "K=4"])
def test_generate_against_the_float64_chain(vf, dev, tabs, case, kind):
    from view_fusion_amd import schedule
    g = case["gpu"]
    if kind == "full":
        kw, tau = dict(sample_num=T - 1), np.arange(T)
    else:
        kw, tau = dict(sample_steps=4, eta=1.0), schedule.sample_timesteps(T, 4)
    y, ret, logits, weights, samples = vf.generate(g["y_cond"], case["vc"], g["angle"], y_t=g["y_T"], z_seq=g["z_seq"], **kw)
    hi, lo = (x.astype(np.float32) for x in schedule.variance_tables(tabs["betas"], None if kind == "full" else tau))
    with torch.no_grad():
        states = vlb_ref.chain(case["unet"], tabs["betas"], torch.from_numpy(tabs["gammas"]), "eps", case["y_cond"],
                               case["vc"], case["angle"], case["y_T"], case["z_seq"], tau, hi, lo)
    assert ret.shape[1] == 1 + len(tau)
    err = float((ret[:, 1:].cpu() - states.transpose(0, 1)).abs().max())
    print(f"generate with a learned variance, {kind}: chain max-abs {err:.3e} against the float64 chain")
    assert torch.equal(y, samples) and err <= CHAIN_TOL
    assert logits.shape[2] == 3 and logits.shape[0] == sum(VC) and torch.isfinite(weights).all()     # three logit channels
    # the fixed-variance step on the same weights is another sample
    vf.set_learned_variance(None)
    try:
        other = vf.generate(g["y_cond"], case["vc"], g["angle"], y_t=g["y_T"], z_seq=g["z_seq"],
                            **(dict(sample_steps=T, eta=1.0) if kind == "full" else kw))[4]
    finally:
        vf.set_learned_variance()
    assert float((other - samples).abs().max()) > 10 * CHAIN_TOL


def test_other_solvers_run_the_existing_kernels_and_guidance_is_finite(vf, dev, case):
    from view_fusion_amd import ops
    g = case["gpu"]
    res = {}
    for on in (True, False):
        vf.set_learned_variance(1e-3 if on else None)
        try:
            for kw in (dict(sample_steps=4, solver="dpmpp2m"), dict(sample_steps=4, eta=0.0), dict(sample_steps=4, eta=0.5)):
                ops.st.KERNEL_LOG = []
                try:
                    out = vf.generate(g["y_cond"], case["vc"], g["angle"], y_t=g["y_T"], z_seq=g["z_seq"], use_graph=False, **kw)
                    names = [r[5] for r in ops.st.KERNEL_LOG]
                finally:
                    ops.st.KERNEL_LOG = None
                assert not [n for n in names if "_lv" in n] and names.count("vf_sampler_step") == 4
                res.setdefault(tuple(sorted(kw.items())), []).append((out[4], out[2]))
        finally:
            vf.set_learned_variance()
    for (a, la), (b, lb) in res.values():
        assert torch.equal(a, b)                                        # the same kernels on the same `out`
        assert la.shape[2] == 3 and lb.shape[2] == 6 and torch.equal(la, lb[:, :, 0:3])
    ops.st.KERNEL_LOG = []
    try:
        y, ret, logits, weights, samples = vf.generate(g["y_cond"], case["vc"], g["angle"], seed=5, sample_steps=4, eta=1.0,
                                                       guidance=2.0, use_graph=False)
        names = [r[5] for r in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None
    assert names.count("vf_sampler_step_lv_cfg_rng") == 4 and "vf_sampler_step_cfg_rng" not in names
    assert all(torch.isfinite(x).all() for x in (y, ret, logits, weights)) and logits.shape[:3:2] == (sum(VC), 3)
    # p_sample / p_mean_variance: the learned step, its mean and the per-pixel log-variance
    t = torch.full((3,), 7, device=dev)
    y1, lg, w = vf.p_sample(g["y_T"], g["y_cond"], case["vc"], g["angle"], t, z=g["z_seq"][7])
    with torch.no_grad():                                               # (the route p_sample's UNet forward takes)
        mean, lp, lg2, _ = vf.p_mean_variance(g["y_T"], g["y_cond"], case["vc"], g["angle"], t, True)
    assert lp.shape == mean.shape == y1.shape and lg.shape[1] == 3 and torch.equal(lg, lg2)
    want = mean.double() + torch.exp(0.5 * lp.double()) * g["z_seq"][7].double()
    assert rel(y1, want) <= KERNEL_RTOL
    assert torch.isfinite(lp).all() and float(lp.std()) > 0             # per pixel


# ---- 5. Trainer ------------------------------------------------------------------------------------------------------------
TB, TVC, SEED = 4, [1, 3, 2, 2], 11


def _trainer(dev, graph, cfg=NINE, lam=LAM, **kw):
    from view_fusion_amd import train
    m = _model(dev, cfg)
    if lam is not None:
        m.set_learned_variance(lam)
    tr = train.Trainer(m, lr_warmup=1, graph=graph, seed=SEED, **kw)
    tr.it = 0
    return m, tr


def _steps(dev, m, tr, n, first=0):
    out = []
    for s in range(first, first + n):
        loss = tr.step(_batch(dev, TB, TVC, s)).clone()
        out.append((loss, m.last_sample_loss.clone(), m.last_level.clone(), m.last_sample_vlb.clone()))
    return out


def _same(a, b):
    return all(torch.equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


@pytest.mark.parametrize("extras", [False, True])
def test_trainer_graph_replay_equals_eager(dev, extras):
    kw = dict(ema_decay=0.9, max_grad_norm=0.05, loss_bins=4) if extras else {}
    (m_e, tr_e), (m_g, tr_g) = _trainer(dev, False, **kw), _trainer(dev, True, **kw)
    if extras:
        for m in (m_e, m_g):
            m.set_cond_dropout(0.25)
    re_, rg = _steps(dev, m_e, tr_e, 3), _steps(dev, m_g, tr_g, 3)
    assert tr_e.graph_steps == 0 and tr_g.graph_steps == 1 and tr_g.mode == "graph"
    assert _same(re_, rg)
    assert all(torch.equal(p, q) for p, q in zip(m_e.parameters(), m_g.parameters()))
    assert all(torch.isfinite(x).all() for r in rg for x in r)
    if extras:
        assert all(torch.equal(a, b) for a, b in zip(m_e.loss_hist, m_g.loss_hist)) and int(m_g.loss_hist[1].sum()) == 3 * TB
    # set_learned_variance(None) after the capture: the graph is dropped, the next step runs L_simple alone
    for m in (m_e, m_g):
        m.set_learned_variance(None)
    le, lg = tr_e.step(_batch(dev, TB, TVC, 3)).clone(), tr_g.step(_batch(dev, TB, TVC, 3)).clone()
    assert tr_g.graph_steps == 1 and torch.equal(le, lg)                # step 4 ran eagerly
    assert all(torch.equal(p, q) for p, q in zip(m_e.parameters(), m_g.parameters()))


def _grads(m):
    return [p.grad.detach().cpu().numpy().copy() for p in m.parameters()]


def test_trainer_accum_steps_against_the_undivided_batch(dev, tabs):
    """test_gpu_grad_accum.py's rule: |g_A - g_1| <= 4 e + 1e-7 max|g_1| per parameter, e the undivided batch's measured
    distance from the float64 oracle (the oracle UNet in float64 under vlb_ref.hybrid_torch, on the very draws the GPU used)."""
    from oracle import unet_ref, view_fusion_ref as vfr
    from view_fusion_amd import ops, train
    batch = _batch(dev, TB, TVC)
    m1, tr1 = _trainer(dev, False)
    loss1 = float(tr1.step(batch))
    names, g1 = [k for k, _ in m1.named_parameters()], _grads(m1)
    fresh = _model(dev)
    ids = torch.arange(TB, dtype=torch.int64, device=dev) + train.step_sample_ids(1, TB)
    t, _, u = ops.draw_train(SEED, ids, fresh.gammas, want_u=True)
    noise = ops.randn_ids(SEED, ids, ops.diffusion.RNG_TRAIN_NOISE, 0, (3, 16, 16))
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in fresh.denoise_fn.state_dict().items()}
    gam = torch.from_numpy(tabs["gammas"]).double()
    tc, uc = t.cpu(), u.cpu().double().reshape(-1, 1)
    level = (gam[tc].reshape(-1, 1) - gam[tc - 1].reshape(-1, 1)) * uc + gam[tc - 1].reshape(-1, 1)
    y_0, nz = batch["y_0"].cpu().double(), noise.cpu().double()
    y_noisy = level.reshape(-1, 1, 1, 1).sqrt() * y_0 + (1 - level.reshape(-1, 1, 1, 1)).sqrt() * nz
    x, ang_s, lvl_s = vfr.stack_views(batch["y_cond"].cpu().double(), TVC, y_noisy, level, batch["angle"].cpu().double())
    out = unet_ref.unet_forward(sd, NINE, x, ang_s, lvl_s)
    ref, _, _ = vlb_ref.hybrid_torch(out, noise.cpu().numpy(), None, TVC, True, level.reshape(-1).float().numpy(), tc.numpy(),
                                     tabs["c1"], tabs["hi"], tabs["lo"], LAM)
    ref.backward()
    g64 = [sd[k[len("denoise_fn."):]].grad.numpy() for k in names]
    e = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(g1, g64)]
    e_loss = abs(loss1 - float(ref.detach()))
    m2, tr2 = _trainer(dev, False, accum_steps=2)
    loss2 = float(tr2.step(batch))
    worst = (0.0, None)
    for k, g, ga, ek in zip(names, _grads(m2), g1, e):
        diff, bound = float(np.abs(g.astype(np.float64) - ga).max()), 4.0 * ek + 1e-7 * float(np.abs(ga).max())
        worst = max(worst, (diff / bound, k))
    bound = 4.0 * e_loss + 1e-7 * abs(loss1)
    print(f"A=2 loss {loss2:.9g}  A=1 {loss1:.9g}  oracle f64 {float(ref.detach()):.12g}  e {e_loss:.3e}  |diff| "
          f"{abs(loss2 - loss1):.3e}  bound {bound:.3e};  worst gradient diff / bound {worst[0]:.3f} ({worst[1]})")
    for k, g, ga, ek in zip(names, _grads(m2), g1, e):
        assert float(np.abs(g.astype(np.float64) - ga).max()) <= 4.0 * ek + 1e-7 * float(np.abs(ga).max()), k
    assert abs(loss2 - loss1) <= bound
    assert m2.last_sample_vlb.numel() == TB // 2


@pytest.mark.parametrize("objective", [dict(), dict(weighting="min_snr")], ids=["default", "min_snr"])
def test_six_channel_model_is_the_untouched_path(dev, objective):
    """A model that never called the setter against one that turned it on and off again: the same launch list, the same
    bits -- and no launch of the new kernels."""
    from view_fusion_amd import ops
    B = 3
    batch, inj = _batch(dev, B, VC), _inject(dev, B)
    runs = []
    for touch in (False, True):
        m = _model(dev, TINY)
        m.set_loss(**objective)
        if touch:
            m.set_learned_variance(0.5)
            m.set_learned_variance(None)
        ops.st.KERNEL_LOG = []
        try:
            loss = m(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"], **inj)
            loss.backward()
            names = [r[5] for r in ops.st.KERNEL_LOG]
        finally:
            ops.st.KERNEL_LOG = None
        runs.append((loss.detach().cpu(), [p.grad.cpu() for p in m.parameters()], names))
        assert m.last_sample_vlb is None
    (la, ga, na), (lb, gb, nb) = runs
    assert torch.equal(la, lb) and all(torch.equal(x, y) for x, y in zip(ga, gb))
    assert na == nb and not [n for n in na if "_lv" in n]
    assert ("vf_compose_loss_fwd" in na) == bool(objective) and ("vf_compose_fwd" in na) == (not objective)


# ---- 6. the refusals that need a device --------------------------------------------------------------------------------------
def test_refusals_on_the_device(dev, case):
    from view_fusion_amd import _lib, ops
    B = 3
    batch, inj = _batch(dev, B, VC), _inject(dev, B)
    g = case["gpu"]
    args = dict(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"])
    n0 = _lib.N_CALLS
    six = _model(dev, TINY)
    six.set_learned_variance()
    with pytest.raises(ValueError, match="out_channel = 6"):
        six(**args, **inj)
    with pytest.raises(ValueError, match="out_channel = 6"):
        six.generate(g["y_cond"], case["vc"], g["angle"])
    m = _model(dev)
    m.set_learned_variance()
    for kw in (dict(threshold=0.9), dict(guidance=2.0, guidance_rescale=0.5)):
        with pytest.raises(ValueError, match="not built"):
            m.generate(g["y_cond"], case["vc"], g["angle"], sample_steps=4, eta=1.0, **kw)
        with pytest.raises(ValueError, match="not built"):
            m.p_sample(g["y_T"], g["y_cond"], case["vc"], g["angle"], torch.full((3,), 3, device=dev), **kw)
    with pytest.raises(ValueError, match="not built"):
        m(**args, self_cond=torch.zeros_like(batch["y_0"]))
    z = torch.zeros_like(batch["y_0"])
    with pytest.raises(ValueError, match="not built"):
        m(**args, distill_z=z, distill_level=torch.full((B,), 0.5, device=dev), distill_eps=z, distill_x0=z)
    with pytest.raises(ValueError, match="learned-variance"):
        _model(dev).set_distill(m, steps=2)
    with pytest.raises(ValueError, match="learned variance"):
        m.set_level_sampler("loss_aware", bins=4)
    with pytest.raises(ValueError, match="learned variance"):
        m.set_self_cond(0.5)
    zt = _model(dev, NINE, dict(SCHED, zero_terminal_snr=True))
    zt.set_learned_variance()
    with pytest.raises(ValueError, match="zero"):                      # an eps model on a zero-terminal-SNR schedule
        zt.generate(g["y_cond"], case["vc"], g["angle"], sample_steps=3)
    # the ops: six channels are named next to the nine wanted
    off, S, max_v = ops.view_offsets(VC, dev)
    out6 = torch.zeros(S, 6, 16, 16, device=dev)
    t = torch.tensor([1, 2, 3], device=dev)
    with pytest.raises(ValueError, match="got 6 instead of 9"):
        ops.compose_loss(out6, batch["y_0"], off, B, True, torch.full((B,), 0.5, device=dev), vlb=(t, *m._lv_tables(), 1e-3))
    plan = m._lv_plan([3, 7, 11, 15, 19], dev)
    with pytest.raises(ValueError, match="got 6 instead of 9"):
        ops.sampler_step(out6, off, g["y_T"], None, t, plan, B, max_v, True, variance=(plan["hi"], plan["lo"]))
    with pytest.raises(ValueError, match="length"):
        ops.sampler_step(torch.zeros(S, 9, 16, 16, device=dev), off, g["y_T"], None, t, plan, B, max_v, True,
                         variance=(plan["hi"][:3], plan["lo"]))
    assert _lib.N_CALLS == n0                                           # every one of them before any launch
