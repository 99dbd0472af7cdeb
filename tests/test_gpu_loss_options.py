"""The loss options on the GPU (ops.compose_loss, ViewFusion.set_loss, train.Trainer(loss_bins=); the
compose_loss_fwd / _finish / _bwd kernels of csrc/diffusion.hip, specification in csrc/loss_weight.h).

  * op level, against the float64 restatement tests/loss_ref.py: every penalty x every weighting, softmax and mean
    composition, at 8x8 (fewer float4s than one block), 12x20 (not a power of two) and 128x192 at B = 1 (more than
    64 * 256 float4s per sample: the grid-stride loop and all 64 partials).  Tolerances: the ones test_gpu_kernels.py's
    compose-MSE test applies to the same quantities -- loss (and the per-sample loss) 1e-6 relative + 1e-7, d unet_out
    1e-5 of its largest element; the arithmetic is the same plus at most three fp32 roundings per element.  The inputs
    are built so that the float64 |noise_hat - target| >= 1e-2 everywhere (L1's sign is discontinuous at 0); the test
    asserts min |d| >= 1e-3 and excludes no element;
  * the histogram: accumulation across calls, more samples than the finish kernel has threads, more bins than threads;
  * the default objective is untouched: bit-identical loss and gradients, the same launch list;
  * model level: the weighted batch's parameter gradient is sum_b w_b grad(loss_b) / B of three default-path B = 1 runs,
    within 4 x the distance of the undivided DEFAULT batch from its three singles (summation order only, the rule of
    test_gpu_grad_accum.py), both taken as max|diff| / max|gradient| with each maximum over all parameters' elements;
  * Trainer: graph replay == eager bit for bit (loss, parameters, accumulators), loss_by_level against numpy binning,
    accum_steps = 2, and a set_loss() call after capture.
Figures are printed before the assertions (run with -s); profiles/loss_options.md records them."""
import numpy as np
import pytest
import torch

import loss_ref
from conftest import TINY

pytestmark = pytest.mark.gpu
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
SEED = 11                               # its draws at B = 3 and B = 4 give min_snr(1) weights on both sides of 1
WEIGHT_CASES = [(None, 0.0, 0.0), ("min_snr", 5.0, 0.0), ("p2", 1.0, 1.0)]
DELTA = 0.7
SHAPES = {"8x8": ((8, 8), (1, 3, 2)), "12x20": ((12, 20), (1, 3, 2)), "128x192": ((128, 192), (2,))}
LEVELS = {3: [0.95, 0.4, 0.05], 1: [0.95]}       # min_snr(5): w = 5/19 < 1, then 1, 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def close(a, b):
    """The compose-MSE test's loss tolerance, element by element."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) < 1e-6 * np.abs(b) + 1e-7))


_INPUTS = {}


def _inputs(shape, weighting):
    """Fixed-seed unet_out / target / level of one shape, built once: target = noise_hat - d with |d| = 0.01 + |N(0, 1)|
    and a random sign, noise_hat the float64 composition, so the float64 reference has min |d| >= 1e-2 - 1e-6."""
    key = (shape, weighting)
    if key not in _INPUTS:
        (H, W), vc = SHAPES[shape]
        g = torch.Generator().manual_seed(3)
        out = (torch.randn(sum(vc), 6, H, W, generator=g) * 2).numpy()
        nh, _ = loss_ref.compose(out, vc, weighting)
        mag = 0.01 + torch.randn(len(vc), 3, H, W, generator=g).abs().double().numpy()
        sign = np.where(torch.rand(len(vc), 3, H, W, generator=g).numpy() < 0.5, -1.0, 1.0)
        target = (nh - sign * mag).astype(np.float32)
        level = np.array(LEVELS[len(vc)], dtype=np.float32)
        _INPUTS[key] = (out, target, level, vc)
    return _INPUTS[key]


def _run_op(dev, out, target, level, vc, weighting, penalty, kind, a, b, hist=None, gloss=1.7):
    from view_fusion_amd import ops
    off, S, _ = ops.view_offsets(list(vc), dev)
    og = torch.from_numpy(out).to(dev).requires_grad_(True)
    loss, sl = ops.compose_loss(og, torch.from_numpy(target).to(dev), off, len(vc), weighting,
                                torch.from_numpy(level).to(dev), penalty, DELTA, kind, a, b, hist=hist)
    assert not sl.requires_grad and loss.requires_grad
    (loss * gloss).backward()
    return float(loss.detach()), sl.cpu().numpy(), og.grad.cpu().numpy()


# ---- op level --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_compose_loss_against_float64(dev, shape, weighting):
    out, target, level, vc = _inputs(shape, weighting)
    n4 = 3 * out.shape[2] * out.shape[3] // 4
    assert (n4 < 256) if shape == "8x8" else (n4 > 64 * 256) if shape == "128x192" else (n4 % 256 != 0)
    w5 = loss_ref.weights(level, "min_snr", 5.0)
    assert w5[0] < 1 and (len(vc) == 1 or (w5[1] == 1 and w5[2] == 1))
    failures = []
    for penalty in loss_ref.PENALTIES:
        for kind, a, b in WEIGHT_CASES:
            ref = loss_ref.loss(out, target, vc, weighting, level, penalty, DELTA, kind, a, b, gloss=1.7)
            assert np.abs(ref["d"]).min() >= 1e-3                      # L1: no element near the kink, none excluded
            if penalty == "huber":
                frac = float((np.abs(ref["d"]) <= DELTA).mean())
                assert 0.1 < frac < 0.9, frac                          # both branches
            loss, sl, dout = _run_op(dev, out, target, level, vc, weighting, penalty, kind, a, b)
            e_loss = abs(loss - ref["loss"]) / abs(ref["loss"])
            e_sl = float((np.abs(sl - ref["sample_loss"]) / np.abs(ref["sample_loss"])).max())
            e_d = rel(dout, ref["dout"])
            print(f"{shape} softmax={weighting} {penalty:5s} {str(kind):7s}: loss {loss:.9g} (f64 {ref['loss']:.12g}) "
                  f"rel {e_loss:.2e}  sample_loss rel {e_sl:.2e}  dout rel {e_d:.2e}")
            if not (close(loss, ref["loss"]) and close(sl, ref["sample_loss"]) and e_d < 1e-5):
                failures.append((penalty, kind, e_loss, e_sl, e_d))
            if len(vc) > 1:
                assert np.all(dout[0, 3:] == 0), (penalty, kind)       # the single-view sample: zero logit gradient
            if not weighting:
                assert np.all(dout[:, 3:] == 0)
    assert not failures, failures


@pytest.mark.parametrize("weighting", [True, False])
def test_huber_with_a_huge_delta_is_half_the_mse(dev, weighting):
    from view_fusion_amd import ops
    out, target, level, vc = _inputs("12x20", weighting)
    off, S, _ = ops.view_offsets(list(vc), dev)
    tg, lv = torch.from_numpy(target).to(dev), torch.from_numpy(level).to(dev)
    om = torch.from_numpy(out).to(dev).requires_grad_(True)
    lm = ops.compose_mse_loss(om, tg, off, len(vc), weighting)
    (lm * 1.7).backward()
    oh = torch.from_numpy(out).to(dev).requires_grad_(True)
    lh, sl = ops.compose_loss(oh, tg, off, len(vc), weighting, lv, "huber", 1e9)
    (lh * 1.7).backward()
    print(f"mse {float(lm):.9g}  huber(1e9) {float(lh):.9g}  dout rel {rel(oh.grad.cpu().numpy(), 0.5 * om.grad.cpu().numpy()):.2e}")
    assert close(float(lh), 0.5 * float(lm))
    assert rel(oh.grad.cpu().numpy(), 0.5 * om.grad.cpu().numpy()) < 1e-5
    assert close(float(sl.mean()), float(lh))


def test_histogram_accumulates_in_index_order(dev):
    """B = 70 samples (the finish kernel has 64 threads), K = 100 bins (more than its threads), two calls."""
    from view_fusion_amd import ops
    B, K, H = 70, 100, 8
    g = torch.Generator().manual_seed(9)
    out, target = torch.randn(B, 6, H, H, generator=g), torch.randn(B, 3, H, H, generator=g)
    level = torch.rand(B, generator=g)
    level[:4] = torch.tensor([0.0, 1.0, 0.999999, 0.01])              # the ends: bins 0, K - 1, K - 1, 1
    off, _, _ = ops.view_offsets([1] * B, dev)
    hist = (torch.zeros(K, device=dev), torch.zeros(K, device=dev, dtype=torch.int32))
    want_s, want_c = np.zeros(K), np.zeros(K, dtype=np.int64)
    for call, kind in enumerate(("min_snr", None)):
        scale = 1.0 + call
        loss, sl = ops.compose_loss((out * scale).to(dev), target.to(dev), off, B, True, level.to(dev), "mse", 1.0, kind,
                                    5.0, 0.0, hist=hist)
        ref = loss_ref.loss((out * scale).numpy(), target.numpy(), [1] * B, True, level.numpy(), "mse", 1.0, kind, 5.0, 0.0)
        assert close(sl.cpu().numpy(), ref["sample_loss"]) and close(float(loss), ref["loss"])
        # the accumulators against numpy binning of the device's own per-sample losses (unweighted, also under min_snr)
        s, c = loss_ref.histogram(level.numpy(), sl.cpu().numpy(), K)
        want_s, want_c = want_s + s, want_c + c
        got_s, got_c = hist[0].cpu().numpy(), hist[1].cpu().numpy()
        assert np.array_equal(got_c, want_c) and got_c.sum() == B * (call + 1)
        # fp32 sums of at most 2 B terms in another order: n eps sum|x|
        assert np.all(np.abs(got_s - want_s) <= 2 * B * 2.0 ** -24 * np.abs(want_s)), call
    assert want_c[0] >= 2 and want_c[K - 1] >= 4 and (want_c == 0).any()
    with pytest.raises(Exception):                                     # a float count tensor is refused, not reinterpreted
        ops.compose_loss(out.to(dev), target.to(dev), off, B, True, level.to(dev), hist=(hist[0], hist[0]))


# ---- model level -----------------------------------------------------------------------------------------------------
def _model(dev):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": SCHED}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


def _batch(dev, B, vc, s=0):
    from view_fusion_amd import train
    return dict(train.synthetic_batch(B, 3, 16, dev, seed=40 + s), view_count=torch.tensor(vc))


def _grads(vf):
    return [p.grad.detach().cpu().numpy().astype(np.float64) for p in vf.parameters()]


def test_default_set_loss_is_the_untouched_path(dev):
    from view_fusion_amd import ops
    B, vc = 3, [1, 3, 2]
    batch = _batch(dev, B, vc)
    g = torch.Generator().manual_seed(1)
    inj = dict(t=torch.tensor([15, 3, 9]).to(dev), u=torch.rand(B, 1, generator=g).to(dev),
               noise=torch.randn(B, 3, 16, 16, generator=g).to(dev))
    runs = []
    for touch in (False, True):
        vf = _model(dev)
        if touch:
            vf.set_loss(penalty="l1", weighting="p2")
            vf.set_loss()                                               # back to the defaults
        ops.st.KERNEL_LOG = []
        try:
            loss = vf(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"], **inj)
            loss.backward()
            names = [r[5] for r in ops.st.KERNEL_LOG]
        finally:
            ops.st.KERNEL_LOG = None
        runs.append((loss.detach().cpu(), [p.grad.cpu() for p in vf.parameters()], names))
        assert vf.last_sample_loss is None
    (la, ga, na), (lb, gb, nb) = runs
    assert torch.equal(la, lb) and all(torch.equal(x, y) for x, y in zip(ga, gb))
    assert na == nb and "vf_compose_fwd" in na and "vf_compose_mse_bwd" in na
    assert not [n for n in na if n.startswith("vf_compose_loss")]


def test_weighted_batch_gradient_is_the_weighted_sum_of_its_samples(dev):
    from view_fusion_amd import ops
    B, vc = 3, [1, 3, 2]
    batch = _batch(dev, B, vc)
    ids = torch.arange(B, dtype=torch.int64, device=dev) + B
    kw = lambda sl: dict(y_cond=batch["y_cond"][sl], view_count=batch["view_count"][sl], angle=batch["angle"][sl],
                         y_0=batch["y_0"][sl], seed=SEED, sample_ids=ids[sl])
    singles = []
    for b in range(B):                                                  # default path, B = 1
        vf = _model(dev)
        vf(**kw(slice(b, b + 1))).backward()
        singles.append(_grads(vf))
    vf = _model(dev)
    vf(**kw(slice(0, B))).backward()                                    # default path, undivided
    g_def = _grads(vf)
    vf = _model(dev)
    vf.set_loss(weighting="min_snr", snr_gamma=1.0)
    loss = vf(**kw(slice(0, B)))
    loss.backward()
    g_w = _grads(vf)
    _, level, _ = ops.draw_train(SEED, ids, vf.gammas)
    assert torch.equal(level, vf.last_level)
    w = loss_ref.weights(level.cpu().numpy(), "min_snr", 1.0)
    assert w.max() == 1.0 and w.min() < 0.5, w
    assert close(float(loss), float((w * vf.last_sample_loss.cpu().numpy()).mean()))

    def dist(got, wts):
        # largest element of the difference over the largest element of the gradient, both over ALL parameters: some
        # parameters' gradients are zero in exact arithmetic (a conv bias in front of a GroupNorm), so a per-parameter
        # scale would divide rounding noise by rounding noise
        diff = scale = 0.0
        for i, g in enumerate(got):
            want = sum(wts[b] * singles[b][i] for b in range(B)) / B
            diff, scale = max(diff, float(np.abs(g - want).max())), max(scale, float(np.abs(want).max()))
        return diff / scale

    e1, ew = dist(g_def, np.ones(B)), dist(g_w, w)
    print(f"w {w}  default batch vs its singles {e1:.3e}  weighted batch vs weighted singles {ew:.3e}  bound {4 * e1:.3e}")
    assert e1 > 0 and ew <= 4.0 * e1, (ew, e1)
    assert dist(g_w, np.ones(B)) > 100 * e1                              # (the weights do change the gradient)


# ---- Trainer ---------------------------------------------------------------------------------------------------------
TB, TVC, K = 4, [1, 3, 2, 2], 8


def _trainer(dev, graph, loss=True, **kw):
    from view_fusion_amd import train
    vf = _model(dev)
    if loss:
        vf.set_loss(penalty="huber", delta=0.5, weighting="min_snr", snr_gamma=1.0)
    tr = train.Trainer(vf, lr_warmup=1, graph=graph, seed=SEED, **kw)
    tr.it = 0
    return vf, tr


def _steps(dev, vf, tr, n, first=0):
    losses, sls, lvs = [], [], []
    for s in range(first, first + n):
        losses.append(tr.step(_batch(dev, TB, TVC, s)).clone())
        sls.append(vf.last_sample_loss.cpu().numpy().copy())
        lvs.append(vf.last_level.cpu().numpy().copy())
    return losses, sls, lvs


def _check_hist(tr, sls, lvs, n_samples):
    mean, count = tr.loss_by_level()
    mean, count = mean.cpu().numpy(), count.cpu().numpy()
    s, c = loss_ref.histogram(np.concatenate(lvs), np.concatenate(sls), K)
    assert np.array_equal(count, c) and count.sum() == n_samples
    assert np.isnan(mean[c == 0]).all() and (c == 0).any() and (c > 0).sum() >= 2
    got = mean[c > 0].astype(np.float64) * c[c > 0]
    assert np.all(np.abs(got - s[c > 0]) <= (n_samples + 2) * 2.0 ** -24 * s[c > 0])   # fp32 sums in another order
    return count


def test_trainer_graph_replay_equals_eager_and_fills_the_histogram(dev):
    (vf_e, tr_e), (vf_g, tr_g) = _trainer(dev, False, loss_bins=K), _trainer(dev, True, loss_bins=K)
    le, sls, lvs = _steps(dev, vf_e, tr_e, 3)
    lg, sls_g, lvs_g = _steps(dev, vf_g, tr_g, 3)
    assert tr_e.graph_steps == 0 and tr_g.graph_steps == 1 and tr_g.mode == "graph"
    assert all(torch.equal(a, b) for a, b in zip(le, lg))
    assert all(np.array_equal(a, b) for a, b in zip(sls + lvs, sls_g + lvs_g))
    assert all(torch.equal(p, q) for p, q in zip(vf_e.parameters(), vf_g.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(vf_e.loss_hist, vf_g.loss_hist))
    _check_hist(tr_e, sls, lvs, 3 * TB)
    count = _check_hist(tr_g, sls_g, lvs_g, 3 * TB)
    # the returned loss is the weighted mean of what the step handed back
    w = loss_ref.weights(lvs_g[2], "min_snr", 1.0)
    assert w.max() == 1.0 and w.min() < 1.0
    assert close(float(lg[2]), float((w * sls_g[2]).mean()))
    # reset
    mean, c2 = tr_g.loss_by_level(reset=True)
    assert np.array_equal(c2.cpu().numpy(), count)
    assert int(tr_g.loss_by_level()[1].sum()) == 0 and bool(torch.isnan(tr_g.loss_by_level()[0]).all())

    # set_loss after the capture: the next step runs the new objective (eagerly: the graphs are gone), and is captured
    # again later; the eager twin agrees bit for bit throughout
    for vf in (vf_e, vf_g):
        vf.set_loss(penalty="huber", delta=0.5, weighting="p2")
    le, sls, lvs = _steps(dev, vf_e, tr_e, 3, first=3)
    lg, sls_g, lvs_g = _steps(dev, vf_g, tr_g, 3, first=3)
    assert tr_g.graph_steps == 2                                         # steps 4, 5 eager again, step 6 a replay
    assert all(torch.equal(a, b) for a, b in zip(le, lg))
    assert all(torch.equal(p, q) for p, q in zip(vf_e.parameters(), vf_g.parameters()))
    for s in range(3):
        p2 = float((loss_ref.weights(lvs_g[s], "p2", 1.0, 1.0) * sls_g[s]).mean())
        old = float((loss_ref.weights(lvs_g[s], "min_snr", 1.0) * sls_g[s]).mean())
        print(f"step {4 + s}: loss {float(lg[s]):.9g}  p2 predicts {p2:.9g}  (min_snr would give {old:.9g})")
        assert close(float(lg[s]), p2) and not close(float(lg[s]), old)
    _check_hist(tr_g, sls_g, lvs_g, 3 * TB)


def test_trainer_accum_steps_fill_the_same_histogram(dev):
    """accum_steps = 2 at B = 4: the same counts as the undivided step, and a loss within the rule of
    test_gpu_grad_accum.py: 4 e + 1e-7 |loss|, e the undivided step's own distance from float64 (the CPU oracle's UNet in
    float64 on the GPU's own draws, then loss_ref)."""
    from oracle import unet_ref, view_fusion_ref as vfr
    from view_fusion_amd import ops, train
    vf1, tr1 = _trainer(dev, False, loss_bins=K)
    batch = _batch(dev, TB, TVC)
    loss1 = float(tr1.step(batch))
    c1 = tr1.loss_by_level()[1].cpu().numpy()
    vf2, tr2 = _trainer(dev, False, loss_bins=K, accum_steps=2)
    loss2 = float(tr2.step(batch))
    c2 = tr2.loss_by_level()[1].cpu().numpy()
    assert np.array_equal(c1, c2) and c2.sum() == TB
    assert vf2.last_sample_loss.numel() == TB // 2                      # the last micro-batch's

    fresh = _model(dev)
    ids = torch.arange(TB, dtype=torch.int64, device=dev) + train.step_sample_ids(1, TB)
    t, level, u = ops.draw_train(SEED, ids, fresh.gammas, want_u=True)
    noise = ops.randn_ids(SEED, ids, ops.diffusion.RNG_TRAIN_NOISE, 0, (3, 16, 16))
    sd = {k: v.detach().cpu().double() for k, v in fresh.denoise_fn.state_dict().items()}
    g64 = vfr.schedule_buffers(vfr.beta_schedule(**SCHED))["gammas"].double()
    lv64 = ((g64[t.cpu()] - g64[t.cpu() - 1]) * u.cpu().double() + g64[t.cpu() - 1]).reshape(-1, 1)
    with torch.no_grad():
        y_noisy = vfr.q_sample(batch["y_0"].cpu().double(), lv64.reshape(-1, 1, 1, 1), noise.cpu().double())
        x, ang_s, lvl_s = vfr.stack_views(batch["y_cond"].cpu().double(), TVC, y_noisy, lv64,
                                          batch["angle"].cpu().double())
        out = unet_ref.unet_forward(sd, TINY, x, ang_s, lvl_s)
    ref = loss_ref.loss(out.numpy(), noise.cpu().numpy(), TVC, True, level.cpu().numpy(), "huber", 0.5, "min_snr", 1.0)
    e = abs(loss1 - ref["loss"])
    bound = 4.0 * e + 1e-7 * abs(loss1)
    print(f"A=2 loss {loss2:.9g}  A=1 {loss1:.9g}  oracle f64 {ref['loss']:.12g}  e {e:.3e}  |diff| {abs(loss2 - loss1):.3e}  "
          f"bound {bound:.3e}")
    assert e < 1e-4 * abs(loss1)                                        # (the oracle does restate this step)
    assert abs(loss2 - loss1) <= bound


def test_histogram_alone_keeps_the_launch_count(dev):
    """loss_bins with the default objective runs the loss-option kernels in place of the MSE ones, launch for launch; and
    loss_bins=None with the default objective is the parent's launch list."""
    from view_fusion_amd import ops
    lists = []
    for kw in (dict(), dict(loss_bins=K)):
        vf, tr = _trainer(dev, False, loss=False, **kw)
        ops.st.KERNEL_LOG = []
        try:
            tr.step(_batch(dev, TB, TVC))
            lists.append([r[5] for r in ops.st.KERNEL_LOG])
        finally:
            ops.st.KERNEL_LOG = None
    plain, binned = lists
    assert not [n for n in plain if n.startswith("vf_compose_loss")]
    assert plain.count("vf_compose_fwd") == 1 and plain.count("vf_compose_mse_bwd") == 1
    swap = {"vf_compose_fwd": "vf_compose_loss_fwd", "vf_compose_mse_bwd": "vf_compose_loss_bwd"}
    assert [swap.get(n, n) for n in plain] == binned
