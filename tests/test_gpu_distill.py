"""Progressive distillation on the GPU (the head of csrc/diffusion.hip holds the definition): the two kernels against the
float64 restatement of tests/distill_ref.py, the identity "one student step on x~ = the teacher's two steps" on the device,
forward() against the two-step chain through the oracle UNet, the Trainer (graph replay, accum_steps), the untouched default
path and drivers.progressive_distill.

Tolerances: the sampler tests' -- one kernel rel 2e-5 (max|a-b| / max|b|), a chain through the UNet max-abs 1e-3 -- and the
loss tests' close(); "bitwise" is torch.equal."""

import numpy as np
import pytest
import torch

import distill_ref
import loss_ref
import prediction_ref
from conftest import TINY

pytestmark = pytest.mark.gpu
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
T = SCHED["num_timesteps"]
# the loss / prediction tests' shapes: less than one workgroup of float4s; a count that is no multiple of 256; more than
# the 64-chunk grid covers in one pass (the grid-stride loop)
SHAPES = {"8x8": ((8, 8), (1, 3, 2)), "12x20": ((12, 20), (1, 3, 2)), "128x192": ((128, 192), (2,))}
KERNEL_RTOL, CHAIN_TOL = 2e-5, 1e-3
VC = [1, 3, 2]
K_OP = 5
STEPS = {3: [0, 2, 4], 1: [3]}                     # per-sample student steps of the op tests: distinct, i = 0 among them
SCALES = {3: [0.0, 1.0, 2.5], 1: [2.5]}


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


def _betas():
    from view_fusion_amd import schedule
    return np.asarray(schedule.make_beta_schedule(**SCHED), dtype=np.float64)


def _model(dev, sched=SCHED, perturb=None):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    if perturb is not None:                                    # a teacher that is not the student
        g = torch.Generator().manual_seed(perturb)
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.02 * torch.randn(p.shape, generator=g))
    vf = ViewFusion(net.to(dev), {"train": dict(sched)}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


def _batch(dev, B, vc, s=0):
    from view_fusion_amd import train
    return dict(train.synthetic_batch(B, 3, 16, dev, seed=40 + s), view_count=torch.tensor(vc))


def _plan(dev, K, prediction):
    """The device tables of a K-step student of a `prediction` teacher, as set_distill makes them."""
    from view_fusion_amd import schedule
    tabs = schedule.distill_tables(_betas(), K, prediction)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)                         # noqa: E731
    return tabs, {k: f32(v) for k, v in tabs["teacher"].items()}, f32(tabs["w1"]), f32(tabs["w2"])


_INPUTS = {}


def _op_inputs(shape):
    """Fixed-seed inputs of distill_target for one shape, made once and left unchanged: the teacher's raw output with null
    rows, z' / x1 / z_t, levels."""
    if shape not in _INPUTS:
        (H, W), vc = SHAPES[shape]
        B = len(vc)
        g = torch.Generator().manual_seed(23 + H)
        out = torch.randn(sum(vc) + B, 6, H, W, generator=g) * 2
        zp, z_t = (torch.randn(B, 3, H, W, generator=g) for _ in range(2))
        x1 = (torch.randn(B, 3, H, W, generator=g) * 0.8).clamp(-1, 1)
        _INPUTS[shape] = (out, zp, x1, z_t, vc)
    return _INPUTS[shape]


# ---- 1. distill_target against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", prediction_ref.PREDICTIONS)
@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("weighting", [True, False], ids=["softmax", "mean"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_distill_target_against_the_restatement(dev, shape, weighting, cfg, prediction):
    from view_fusion_amd import ops
    out, zp, x1, z_t, vc = _op_inputs(shape)
    B, S = len(vc), sum(vc)
    n4 = 3 * out.shape[2] * out.shape[3] // 4
    assert (n4 < 256) if shape == "8x8" else (n4 > 64 * 256) if shape == "128x192" else (n4 % 256 != 0)
    betas = _betas()
    tabs, plan, w1, w2 = _plan(dev, K_OP, prediction)
    i = np.array(STEPS[B])
    gam32 = np.cumprod(1.0 - betas).astype(np.float32)
    level = gam32[tabs["tau_s"][i]]
    scales = SCALES[B] if cfg else None
    rows = out if cfg else out[:S]
    comp, _ = loss_ref.compose(rows[:S].numpy(), vc, weighting)
    comp = distill_ref.guided(comp, rows[S:, :3].numpy(), scales) if cfg else comp
    want_x2, want_x, want_e = distill_ref.second_step(betas, K_OP, prediction, i, level, zp.numpy(), x1.numpy(), z_t.numpy(),
                                                       comp)
    off, _, max_v = ops.view_offsets(list(vc), dev)
    it = torch.tensor(i, device=dev)
    k0 = 2 * it
    gs = torch.tensor(scales, dtype=torch.float32, device=dev) if cfg else None
    args = (rows.to(dev), off, zp.to(dev), x1.to(dev), z_t.to(dev), torch.from_numpy(level).to(dev), it, k0, plan, w1, w2, B,
            weighting)
    x_t, e_t = ops.distill_target(*args, guidance=gs, S=S)
    ex, ee = rel(x_t, want_x), rel(e_t, want_e)
    print(f"{shape} {'softmax' if weighting else 'mean'} {'cfg' if cfg else 'plain'} {prediction}: x~ rel {ex:.2e}  "
          f"eps~ rel {ee:.2e}  |x~| max {float(x_t.abs().max()):.7f}  clamped share {float((x_t.abs() == 1).float().mean()):.2f}")
    assert torch.isfinite(x_t).all() and torch.isfinite(e_t).all()
    assert ex <= KERNEL_RTOL and ee <= KERNEL_RTOL
    assert float(x_t.abs().max()) <= 1.0                                  # within [-1, 1] exactly
    # the same bits on a second call: no atomics
    x_b, e_b = ops.distill_target(*args, guidance=gs, S=S)
    assert torch.equal(x_t, x_b) and torch.equal(e_t, e_b)
    # i = 0: x~ is x2 to the bit -- the y0 the few-step tail itself writes for step k0, whatever the history holds
    zero = [b for b in range(B) if i[b] == 0]
    if zero:
        hist = torch.empty_like(x_t)
        ops.sampler_step(rows.to(dev), off, zp.to(dev), None, k0, plan, B, max_v, weighting, y0_prev=hist,
                         want_weights=False, guidance=gs, S=S)
        other = list(args)
        other[3] = -x1.to(dev)
        x_o, _ = ops.distill_target(*other, guidance=gs, S=S)
        for b in zero:
            assert rel(hist[b], want_x2[b]) <= KERNEL_RTOL
            assert torch.equal(x_t[b], hist[b]) and torch.equal(x_o[b], x_t[b])
        assert not torch.equal(x_o, x_t)


def test_distill_target_argument_errors(dev):
    from view_fusion_amd import ops
    out, zp, x1, z_t, vc = _op_inputs("8x8")
    _, plan, w1, w2 = _plan(dev, K_OP, "eps")
    off, S, _ = ops.view_offsets(list(vc), dev)
    it = torch.tensor([0, 2, 4], device=dev)
    lv = torch.full((3,), 0.5, device=dev)
    good = [out[:S].to(dev), off, zp.to(dev), x1.to(dev), z_t.to(dev), lv, it, 2 * it, plan, w1, w2, 3, True]
    ops.distill_target(*good)
    for pos, bad in ((0, out.to(dev)[:S, :3].contiguous()), (3, x1.to(dev)[:2]), (6, it.int()), (9, w1[:4]), (5, lv[:2])):
        args = list(good)
        args[pos] = bad
        with pytest.raises((ValueError, RuntimeError)):
            ops.distill_target(*args)
    with pytest.raises(ValueError):                                       # guided: S + B rows
        ops.distill_target(*good, guidance=torch.ones(3, device=dev), S=S)


# ---- 2. distill_begin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_distill_begin(dev, shape):
    from view_fusion_amd import ops
    (H, W), vc = SHAPES[shape]
    B = len(vc)
    g = torch.Generator().manual_seed(5 + H)
    y_0, noise = torch.rand(B, 3, H, W, generator=g) * 2 - 1, torch.randn(B, 3, H, W, generator=g)
    vf = _model(dev)
    betas = _betas()
    for K in (1, 4, 10):
        tau_s = torch.tensor(distill_ref.timesteps(T, K), device=dev)
        # injected i (clamped into range before any table is read)
        inj = torch.tensor([0, K + 3, K // 2] if B > 1 else [K + 3], device=dev)
        want_i = inj.clamp(0, K - 1)
        i, k1, k0, level, z_t = ops.distill_begin(y_0.to(dev), noise.to(dev), tau_s, vf.gammas, i=inj)
        assert i.dtype == k1.dtype == k0.dtype == torch.int64
        assert torch.equal(i, want_i) and torch.equal(k1, 2 * want_i + 1) and torch.equal(k0, 2 * want_i)
        assert torch.equal(level, vf.gammas[tau_s[want_i]])
        lv, want_z = distill_ref.begin(vf.gammas.cpu().numpy(), tau_s.cpu().numpy(), want_i.cpu().numpy(), y_0.numpy(),
                                       noise.numpy())
        assert np.array_equal(lv, level.cpu().numpy())
        e = rel(z_t, want_z)
        print(f"{shape} K {K}: z_t rel {e:.2e}")
        assert e <= KERNEL_RTOL
        # the student's stacked target half is this buffer, bit for bit
        off, S, _ = ops.view_offsets(list(vc), dev)
        y_cond = torch.rand(B, max(vc), 3, H, W, generator=g).to(dev)
        x, level_s, _ = ops.stack_views(y_cond, z_t, None, level, torch.zeros(B, 1, device=dev), off, S)
        rows = torch.repeat_interleave(torch.arange(B), torch.tensor(vc)).to(dev)
        assert torch.equal(x[:, 3:], z_t[rows]) and torch.equal(level_s.reshape(-1), level[rows])
        # the seeded draw is the host mirror's, whatever the batch
        seed, ids = 0xD15717, torch.tensor([7, 2 ** 33 + 1, 12][:B], device=dev)
        i_s, k1_s, k0_s, level_s2, z_s = ops.distill_begin(y_0.to(dev), noise.to(dev), tau_s, vf.gammas, seed=seed, ids=ids)
        host = ops.distill_step_host(seed, ids.cpu(), K)
        assert torch.equal(i_s.cpu(), host) and np.array_equal(host.numpy(), distill_ref.draw_step(seed, ids.cpu().numpy(), K))
        assert torch.equal(k1_s, 2 * i_s + 1) and torch.equal(k0_s, 2 * i_s) and torch.equal(level_s2, vf.gammas[tau_s[i_s]])
        again = ops.distill_begin(y_0.to(dev), noise.to(dev), tau_s, vf.gammas, i=i_s)
        assert torch.equal(again[4], z_s)
    with pytest.raises(ValueError):
        ops.distill_begin(y_0.to(dev), noise.to(dev), tau_s, vf.gammas)
    with pytest.raises(ValueError):
        ops.distill_begin(y_0.to(dev), noise.to(dev), tau_s, vf.gammas, seed=1, i=inj)


# ---- 3. the identity on the device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", prediction_ref.PREDICTIONS)
def test_student_step_on_the_target_is_the_teachers_two_steps(dev, prediction):
    from view_fusion_amd import ops
    (H, W), vc = SHAPES["12x20"]
    B, S = 3, sum(vc)
    g = torch.Generator().manual_seed(77)
    out1, out2 = (torch.randn(S, 6, H, W, generator=g).to(dev) for _ in range(2))
    z_t = torch.randn(B, 3, H, W, generator=g).to(dev)
    tabs, plan, w1, w2 = _plan(dev, K_OP, prediction)
    it = torch.tensor([0, 2, 4], device=dev)
    k1, k0 = 2 * it + 1, 2 * it
    off, _, max_v = ops.view_offsets(list(vc), dev)
    gam32 = np.cumprod(1.0 - _betas()).astype(np.float32)
    level = torch.from_numpy(gam32[tabs["tau_s"][it.cpu().numpy()]]).to(dev)
    x1 = torch.empty_like(z_t)
    zp, _ = ops.sampler_step(out1, off, z_t, None, k1, plan, B, max_v, True, y0_prev=x1, want_weights=False)
    zpp, _ = ops.sampler_step(out2, off, zp, None, k0, plan, B, max_v, True, want_weights=False)
    x_t, e_t = ops.distill_target(out2, off, zp, x1, z_t, level, it, k0, plan, w1, w2, B, True)
    i = it.cpu().numpy()
    cy, c0 = tabs["student"]["cy"][i].reshape(-1, 1, 1, 1), tabs["student"]["c0"][i].reshape(-1, 1, 1, 1)
    got = cy * z_t.double().cpu().numpy() + c0 * x_t.double().cpu().numpy()
    e = rel(got, zpp)
    # ... and eps~ is the noise that carries x~ to z_t at the student's level
    lv = level.double().cpu().numpy().reshape(-1, 1, 1, 1)
    back = np.sqrt(lv) * x_t.double().cpu().numpy() + np.sqrt(1 - lv) * e_t.double().cpu().numpy()
    e2 = rel(back, z_t)
    print(f"{prediction}: cy_S z_t + c0_S x~ against the teacher's z'' rel {e:.2e}; sqrt(g) x~ + sqrt(1-g) eps~ against z_t rel {e2:.2e}")
    assert e <= KERNEL_RTOL and e2 <= KERNEL_RTOL


# ---- 4. model level ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle(dev):
    """The teacher's weights and their CPU oracle, made once and left unchanged."""
    from oracle import unet_ref
    teacher = _model(dev, perturb=5)
    sd = {k: v.detach().cpu().clone() for k, v in teacher.denoise_fn.state_dict().items()}
    return dict(sd=sd, unet=lambda x, a, l: unet_ref.unet_forward(sd, TINY, x, a, l))


def _teacher(dev, oracle, prediction="eps"):
    t = _model(dev)
    t.denoise_fn.load_state_dict(oracle["sd"])
    t.set_prediction(prediction)
    return t


def _ref_two_steps(oracle, batch, K, prediction, i, noise, guidance=None, weighting=True):
    """The float64 two-step chain through the oracle UNet (fp32 network, float64 everything after it)."""
    from oracle import view_fusion_ref as vfr
    import guidance_ref
    y_cond, angle, vc = batch["y_cond"].cpu(), batch["angle"].cpu(), [int(v) for v in batch["view_count"]]
    S, B = sum(vc), len(vc)
    betas = _betas()
    gam32 = vfr.schedule_buffers(vfr.beta_schedule(**SCHED))["gammas"].numpy()

    def teacher(y, level):
        lv = torch.tensor(level, dtype=torch.float32).reshape(B, 1)
        with torch.no_grad():
            x, ang_s, lvl_s = guidance_ref.stack(y_cond, vc, torch.tensor(y).float(), lv, angle, null_rows=guidance is not None)
            out = oracle["unet"](x[:S], ang_s[:S], lvl_s[:S])
            comp, _ = loss_ref.compose(out.double().numpy(), vc, weighting)
            if guidance is None:
                return comp
            null = oracle["unet"](x[S:], ang_s[S:], lvl_s[S:])
        return distill_ref.guided(comp, null[:, :3].double().numpy(), np.full(B, guidance, dtype=np.float32))

    return distill_ref.two_steps(betas, gam32, K, prediction, i, batch["y_0"].cpu().numpy(), noise.cpu().numpy(), teacher)


MODEL_CASES = [dict(K=4, student="eps", teacher="eps"), dict(K=10, student="v", teacher="eps"),
               dict(K=4, student="x0", teacher="v"), dict(K=10, student="eps", teacher="eps", loss="trunc_snr"),
               dict(K=4, student="eps", teacher="eps", guidance=2.0)]


@pytest.mark.parametrize("case", MODEL_CASES, ids=["eps-K4", "v-K10", "x0-vteacher-K4", "trunc_snr-K10", "guided-K4"])
def test_forward_against_the_two_step_chain(dev, oracle, case):
    from view_fusion_amd import ops
    K, B, seed = case["K"], 3, 31
    student = _model(dev)
    student.set_prediction(case["student"])
    if case.get("loss"):
        student.set_loss(weighting=case["loss"])
    teacher = _teacher(dev, oracle, case["teacher"])
    before = [p.detach().clone() for p in teacher.parameters()]
    student.set_distill(teacher, steps=K, guidance=case.get("guidance"))
    student.train()
    batch = _batch(dev, B, VC)
    ids = torch.tensor([3, 2 ** 33 + 9, 14], device=dev)
    seen = {}
    hook = student.denoise_fn.register_forward_pre_hook(lambda m, a: seen.update(x=a[0].clone(), level=a[2].clone()))
    loss = student(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"],
                   seed=seed, sample_ids=ids)
    hook.remove()
    loss.backward()
    i, x_t = student.last_distill
    assert torch.equal(i.cpu(), ops.distill_step_host(seed, ids.cpu(), K))
    noise = ops.randn_ids(seed, ids, ops.diffusion.RNG_TRAIN_NOISE, 0, (3, 16, 16))
    ref = _ref_two_steps(oracle, batch, K, case["teacher"], i.cpu().numpy(), noise, case.get("guidance"))
    err = float(np.abs(x_t.double().cpu().numpy() - ref["x_tilde"]).max())
    # what the student saw: z_t and gammas[tau_S[i]], bit for bit
    tgt = student.distill_targets(batch["y_cond"], batch["view_count"], batch["angle"], batch["y_0"], seed=seed,
                                  sample_ids=ids)
    rows = torch.repeat_interleave(torch.arange(B), torch.tensor(VC)).to(dev)
    tau_s = torch.tensor(distill_ref.timesteps(T, K), device=dev)
    assert torch.equal(tgt["distill_x0"], x_t) and torch.equal(seen["x"][:, 3:], tgt["distill_z"][rows])
    assert torch.equal(seen["level"].reshape(-1), student.gammas[tau_s[i]][rows])
    assert torch.equal(tgt["distill_level"], student.gammas[tau_s[i]])
    ez = rel(tgt["distill_z"], ref["z_t"])
    ee = float(np.abs(tgt["distill_eps"].double().cpu().numpy() - ref["eps_tilde"]).max())
    # the loss is the existing objective on the device's own (eps~, x~)
    with torch.no_grad():
        off, S, _ = ops.view_offsets(batch["view_count"], dev)
        out = student.denoise_fn(seen["x"], torch.repeat_interleave(batch["angle"], torch.tensor(VC).to(dev), dim=0),
                                 seen["level"])
        pred = {} if case["student"] == "eps" else dict(prediction=case["student"], y_0=tgt["distill_x0"])
        want, sl = ops.compose_loss(out, tgt["distill_eps"], off, B, True, tgt["distill_level"],
                                    weight_kind=case.get("loss"), **pred)
    print(f"{case}: i {i.tolist()}  x~ max-abs {err:.3e} against the float64 chain (eps~ {ee:.3e}, z_t rel {ez:.2e})  "
          f"loss {float(loss.detach()):.9g}  compose_loss on (eps~, x~) {float(want):.9g}")
    assert err <= CHAIN_TOL and ez <= KERNEL_RTOL
    assert close(float(loss.detach()), float(want))
    if case.get("loss") or case["student"] != "eps":
        assert close(student.last_sample_loss.cpu().numpy(), sl.cpu().numpy())
        assert torch.equal(student.last_level, tgt["distill_level"])
    # the teacher: unchanged bit for bit, no gradient; the student has one
    assert all(torch.equal(p, q) for p, q in zip(teacher.parameters(), before))
    assert all(p.grad is None for p in teacher.parameters()) and not teacher.training
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in student.parameters())
    # injected t is read as i; an injected noise wins
    loss_i = student(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"],
                     t=i, noise=noise)
    assert torch.equal(loss_i.detach(), loss.detach())
    # in eval mode the plain objective runs
    last = student.last_distill
    student.eval()
    student(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"], seed=seed)
    assert student.last_distill is last


# ---- 5. Trainer ------------------------------------------------------------------------------------------------------------
TB, TVC, SEED = 4, [1, 3, 2, 2], 11


def _trainer(dev, oracle, graph, K=4, **kw):
    from view_fusion_amd import train
    vf = _model(dev)
    teacher = _teacher(dev, oracle)
    vf.set_distill(teacher, steps=K)
    tr = train.Trainer(vf, lr_warmup=1, graph=graph, seed=SEED, **kw)
    tr.it = 0
    return vf, teacher, tr


def _steps(dev, vf, tr, n, first=0):
    out = []
    for s in range(first, first + n):
        loss = tr.step(_batch(dev, TB, TVC, s)).clone()
        out.append((loss, vf.last_distill[0].clone(), vf.last_distill[1].clone()))
    return out


def _same(a, b):
    return all(torch.equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def test_trainer_graph_replay_equals_eager(dev, oracle):
    (vf_e, t_e, tr_e), (vf_g, t_g, tr_g) = _trainer(dev, oracle, False), _trainer(dev, oracle, True)
    before = [p.detach().clone() for p in t_g.parameters()]
    re_, rg = _steps(dev, vf_e, tr_e, 4), _steps(dev, vf_g, tr_g, 4)
    assert tr_e.graph_steps == 0 and tr_g.graph_steps == 2 and tr_g.mode == "graph"
    assert _same(re_, rg)
    assert all(torch.equal(p, q) for p, q in zip(vf_e.parameters(), vf_g.parameters()))
    assert len({float(r[0]) for r in rg}) == 4
    # the optimizer holds the student's parameters only; the teacher has not moved
    held = {id(p) for grp in tr_g.opt.param_groups for p in grp["params"]}
    assert held == {id(p) for p in vf_g.parameters()} and not any(id(p) in held for p in t_g.parameters())
    assert all(torch.equal(p, q) for p, q in zip(t_g.parameters(), before))
    assert all(p.grad is None for p in t_g.parameters())
    # set_distill(None) after the capture: the captured step is dropped, the plain objective runs
    plain = _model(dev)
    plain.load_state_dict(vf_g.state_dict())
    from view_fusion_amd import train
    tr_p = train.Trainer(plain, lr_warmup=1, graph=False, seed=SEED)
    tr_p.it = tr_g.it
    for m in (vf_e, vf_g):
        m.set_distill(None)
    n = tr_g.graph_steps
    bt = _batch(dev, TB, TVC, 9)
    le, lg, lp = tr_e.step(bt), tr_g.step(bt), tr_p.step(bt)
    assert tr_g.graph_steps == n and vf_g.last_distill is None
    assert torch.equal(le, lg) and torch.equal(lg, lp)


def test_trainer_accum_steps(dev, oracle):
    (vf_e, _, tr_e), (vf_g, _, tr_g) = _trainer(dev, oracle, False, accum_steps=2), _trainer(dev, oracle, True, accum_steps=2)
    (vf_1, _, tr_1) = _trainer(dev, oracle, False)
    re_, rg, r1 = _steps(dev, vf_e, tr_e, 3), _steps(dev, vf_g, tr_g, 3), _steps(dev, vf_1, tr_1, 3)
    assert tr_g.graph_steps >= 1 and _same(re_, rg)
    assert all(torch.equal(p, q) for p, q in zip(vf_e.parameters(), vf_g.parameters()))
    # a micro-batch targets what its samples target in the undivided batch: the last one holds samples 2, 3.  The draw is
    # an integer and equal; x~ went through the teacher's UNet in another batch (another split of the same sums), so it
    # and the loss are compared at the suite's bound for a chain through the UNet
    assert vf_g.last_distill[0].numel() == TB // 2
    assert torch.equal(rg[0][1], r1[0][1][TB // 2:])
    ex = float((rg[0][2] - r1[0][2][TB // 2:]).abs().max())
    el = abs(float(rg[0][0]) - float(r1[0][0])) / abs(float(r1[0][0]))
    print(f"accum_steps 2 against the undivided batch, step 0: x~ max-abs {ex:.3e}  loss rel {el:.3e}")
    assert ex <= CHAIN_TOL and el <= CHAIN_TOL


# ---- 6. defaults untouched -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", [dict(), dict(weighting="min_snr")], ids=["default", "min_snr"])
def test_the_default_step_is_untouched(dev, oracle, objective):
    from view_fusion_amd import ops
    B = 3
    batch = _batch(dev, B, VC)
    g = torch.Generator().manual_seed(1)
    inj = dict(t=torch.tensor([15, 3, 9]).to(dev), u=torch.rand(B, 1, generator=g).to(dev),
               noise=torch.randn(B, 3, 16, 16, generator=g).to(dev))
    runs = []
    for touch in ("never", "none", "set-unset"):
        vf = _model(dev)
        vf.set_loss(**objective)
        if touch == "none":
            vf.set_distill(None)
        elif touch == "set-unset":
            vf.set_distill(_teacher(dev, oracle), steps=4, guidance=2.0)
            vf.set_distill(None)
        vf.train()
        ops.st.KERNEL_LOG = []
        try:
            loss = vf(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"], **inj)
            loss.backward()
            names = [r[5] for r in ops.st.KERNEL_LOG]
        finally:
            ops.st.KERNEL_LOG = None
        runs.append((loss.detach().cpu(), [p.grad.cpu() for p in vf.parameters()], names))
    for lb, gb, nb in runs[1:]:
        assert torch.equal(runs[0][0], lb) and all(torch.equal(x, y) for x, y in zip(runs[0][1], gb)) and nb == runs[0][2]
    names = runs[0][2]
    assert not [n for n in names if "distill" in n or "sampler_step" in n]
    glue = [n for n in names if n in ("vf_gather_level", "vf_stack_views", "vf_compose_fwd", "vf_compose_mse_bwd",
                                      "vf_compose_loss_fwd", "vf_compose_loss_bwd", "vf_draw_train", "vf_randn_ids")]
    loss_pair = ["vf_compose_loss_fwd", "vf_compose_loss_bwd"] if objective else ["vf_compose_fwd", "vf_compose_mse_bwd"]
    assert glue == ["vf_gather_level", "vf_stack_views"] + loss_pair
    if objective:                                    # min_snr's weights with the new kind compiled in
        lv = ops.gather_level(vf.gammas, inj["t"], inj["u"].reshape(-1).contiguous()).cpu().numpy()
        _, _, w = ops.compose_loss(torch.zeros(sum(VC), 6, 16, 16, device=dev), inj["noise"], ops.view_offsets(VC, dev)[0], B,
                                   True, torch.from_numpy(lv).to(dev), weight_kind="min_snr", a=5.0, want_weight=True)
        assert close(w.cpu().numpy(), loss_ref.weights(lv, "min_snr", 5.0))
        assert close(w.cpu().numpy(), ops.loss_weights_pred_host(lv, "eps", "min_snr", 5.0).numpy())


def test_trunc_snr_on_the_device(dev):
    from view_fusion_amd import ops
    level = np.array([0.95, 0.4, 0.05], dtype=np.float32)
    g = torch.Generator().manual_seed(3)
    out = torch.randn(sum(VC), 6, 8, 8, generator=g).to(dev)
    noise, y_0 = torch.randn(3, 3, 8, 8, generator=g).to(dev), torch.randn(3, 3, 8, 8, generator=g).to(dev)
    off = ops.view_offsets(VC, dev)[0]
    for prediction in prediction_ref.PREDICTIONS:
        pred = {} if prediction == "eps" else dict(prediction=prediction, y_0=y_0)
        loss, sl, w = ops.compose_loss(out, noise, off, 3, True, torch.from_numpy(level).to(dev), weight_kind="trunc_snr",
                                       want_weight=True, **pred)
        w64 = distill_ref.trunc_snr(level, prediction)
        host = ops.loss_weights_pred_host(level, prediction, "trunc_snr").numpy()
        print(f"trunc_snr {prediction}: device {w.cpu().numpy()}  host {host}  f64 {w64}")
        assert close(w.cpu().numpy(), w64) and close(w.cpu().numpy(), host)
        assert close(float(loss), float((w64 * sl.double().cpu().numpy()).mean()))


# ---- 7. the driver ---------------------------------------------------------------------------------------------------------
def test_progressive_distill_two_stages(dev, oracle):
    from view_fusion_amd import drivers, train
    vf, teacher = _model(dev), _teacher(dev, oracle)
    tr = train.Trainer(vf, lr_warmup=1, graph=False, seed=SEED)
    calls, snaps = [], []
    orig = vf.set_distill

    def spy(t=None, steps=None, guidance=None, **kw):
        if calls:                                     # the teacher now holds what the student was when the stage ended
            snaps.append(all(torch.equal(p, q) for p, q in zip(teacher.parameters(), vf.parameters())))
        calls.append((t, steps, guidance))
        return orig(t, steps=steps, guidance=guidance, **kw)

    vf.set_distill = spy
    ptrs = [p.data_ptr() for p in teacher.parameters()]
    out = drivers.progressive_distill(tr, teacher, (_batch(dev, TB, TVC, s) for s in range(4)), start_steps=8, end_steps=2,
                                      iters_per_stage=2, guidance=2.0)
    assert [c[1] for c in calls] == [4, 2] and [c[2] for c in calls] == [2.0, None] and all(c[0] is teacher for c in calls)
    assert snaps == [True] and [k for k, _ in out] == [4, 2]
    assert all(torch.isfinite(l) and l.is_cuda and l.dim() == 0 for _, l in out)
    assert tr.it == 3
    # after the last swap too: the teacher is the student bit for bit, in the tensors it always had
    assert all(torch.equal(p, q) for p, q in zip(teacher.parameters(), vf.parameters()))
    assert [p.data_ptr() for p in teacher.parameters()] == ptrs
    assert vf._distill["steps"] == 2 and vf._distill["guidance"] is None
    batch = _batch(dev, 3, VC)
    y, ret, _, _, samples = vf.generate(batch["y_cond"], batch["view_count"], batch["angle"], seed=5, sample_steps=2)
    assert torch.isfinite(ret).all() and torch.isfinite(samples).all() and float(samples.abs().max()) <= 1.0
