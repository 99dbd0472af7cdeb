"""Gradient accumulation on the GPU (train.Trainer(accum_steps=A), optim.FusedAdam.accumulate, the vf_grad_accum_multi
launch of csrc/adam.hip).

  * the launch through the C ABI, bit-equal to tests/accum_ref.py (float4 tails, block boundaries, a NaN-filled
    accumulator that the first call must not read, guard words around every tensor);
  * A = 1 is the path without the argument: no accumulate launch, the same parameters bit for bit;
  * the plumbing is exact: the accumulated p.grad is accum_ref applied to the micro-batches' own gradients, the
    parameters are FusedAdam's step on it, both bit for bit;
  * A = 2 and A = 4 against the undivided batch within 4 e + 1e-7 max|g| per parameter, e MEASURED per parameter: the max
    abs difference between the A = 1 GPU gradient and the CPU oracle's gradient for the same inputs in float64, i.e. the
    fp32 noise of one summation order against another (the micro-batches only re-associate the sums over the stacked
    views, so their distance from the undivided batch is a difference of two such noises).  The loss under the same
    rule.  Figures are printed before the assertions (run with -s); profiles/grad_accum.md records them;
  * graph replay == eager launches bit for bit; max_grad_norm / ema_decay act on the accumulated gradient, once per step.
"""
import ctypes

import numpy as np
import pytest
import torch

import accum_ref
import optim_ref
from conftest import TINY

pytestmark = pytest.mark.gpu
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
B, N, HW, SEED = 4, 3, 16, 11
VC = [1, 3, 2, 2]                       # ragged: the micro-batches of A = 2 stack 4 + 4 views, of A = 4 1 / 3 / 2 / 2
SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4099)
GUARD = 4                               # floats of guard on either side of every tensor (keeps 16-byte alignment)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the launch through the C ABI ----------------------------------------------------------------------------------
def test_accumulate_launch_is_bit_equal_to_the_restatement(dev):
    from view_fusion_amd import _lib
    rng = np.random.default_rng(0)
    grads = [[rng.standard_normal(n).astype(np.float32) for n in SIZES] for _ in range(3)]
    offs, total = [], 0
    for n in SIZES:                                            # [guard | tensor | pad to 4 | guard] ...
        total += GUARD
        offs.append(total)
        total += (n + 3) // 4 * 4
    total += GUARD
    acc = torch.full((total,), float("nan"), device=dev)       # guards AND payload: the first call must not read it
    g = torch.zeros(total, device=dev)
    rows, first = [], 0
    for n, o in zip(SIZES, offs):
        rows.append([acc.data_ptr() + 4 * o, g.data_ptr() + 4 * o, 0, 0, n, first])
        first += (n + 1023) // 1024
    assert all(r[0] % 16 == 0 and r[1] % 16 == 0 for r in rows)
    desc = torch.tensor(rows, dtype=torch.int64).to(dev)
    scal = torch.zeros(4, device=dev)
    raw = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    w = 1.0 / 3.0
    for call, gs in enumerate(grads):
        host = np.zeros(total, dtype=np.float32)
        for n, o, a in zip(SIZES, offs, gs):
            host[o:o + n] = a
        g.copy_(torch.from_numpy(host))
        _lib.call("vf_adam_set_scalars", ctypes.c_void_p(scal.data_ptr()), 0.0 if call == 0 else 1.0, w, 0.0, raw)
        _lib.call("vf_grad_accum_multi", ctypes.c_void_p(desc.data_ptr()), len(SIZES), first,
                  ctypes.c_void_p(scal.data_ptr()), raw)
        got = acc.cpu().numpy()
        want = accum_ref.accumulate_all(grads[:call + 1], [w] * (call + 1))
        covered = np.zeros(total, dtype=bool)
        for n, o, a in zip(SIZES, offs, want):
            assert np.array_equal(_bits(got[o:o + n]), _bits(a)), (call, n)
            covered[o:o + n] = True
        assert np.all(np.isnan(got[~covered])), call            # nothing outside a tensor's numel was written
    assert not np.isnan(got[covered]).any()


# ---- Trainer ---------------------------------------------------------------------------------------------------------
def _model(dev):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": SCHED}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


def _trainer(dev, graph, **kw):
    from view_fusion_amd import train
    vf = _model(dev)
    tr = train.Trainer(vf, lr_warmup=1, graph=graph, seed=SEED, **kw)
    tr.it = 0                                      # (lr = peak from the first iteration on; the first step is it = 1)
    return vf, tr


def _batch(dev, s=0):
    from view_fusion_amd import train
    return dict(train.synthetic_batch(B, N, HW, dev, seed=40 + s), view_count=torch.tensor(VC))


def _params(vf):
    return [p.detach().cpu().clone() for p in vf.parameters()]


def _grads(vf):
    return [p.grad.detach().cpu().numpy().copy() for p in vf.parameters()]


def _first_ids(dev):
    from view_fusion_amd import train
    return torch.arange(B, dtype=torch.int64, device=dev) + train.step_sample_ids(1, B)


def test_one_accum_step_is_the_path_without_the_argument(dev, monkeypatch):
    from view_fusion_amd import _lib, ops
    names, real = [], _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    (vf_a, tr_a), (vf_b, tr_b) = _trainer(dev, True), _trainer(dev, True, accum_steps=1)
    for s in range(3):
        la, lb = tr_a.step(_batch(dev, s)), tr_b.step(_batch(dev, s))
        assert torch.equal(la, lb)
    torch.cuda.synchronize()
    assert "vf_grad_accum_multi" not in names
    assert tr_a.graph_steps == tr_b.graph_steps == 1
    assert all(torch.equal(a, b) for a, b in zip(_params(vf_a), _params(vf_b)))
    # the two trainers' optimizer launches, interleaved: two eager steps, the capture, one replay -- each
    opt_names = [n for n in names if n.startswith(("vf_adam", "vf_grad_", "vf_swap"))]
    assert opt_names == ["vf_adam_multi"] * 4 + ["vf_adam_multi_dev", "vf_adam_set_scalars"] * 2, opt_names
    # the kernel-log idiom (an eager, instrumented step): the optimizer's launches are the one old entry point
    ops.st.KERNEL_LOG = []
    try:
        tr_b.step(_batch(dev, 3))
        logged = [r[5] for r in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None
    assert [n for n in logged if n.startswith(("vf_adam", "vf_grad_", "vf_swap"))] == ["vf_adam_multi"], logged
    # ... and with accum_steps = 2 the new launch is there, once per micro-batch, in front of the same Adam launch
    vf_c, tr_c = _trainer(dev, True, accum_steps=2)
    ops.st.KERNEL_LOG = []
    try:
        tr_c.step(_batch(dev, 0))
        logged = [r[5] for r in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None
    assert [n for n in logged if n.startswith(("vf_adam", "vf_grad_", "vf_swap"))] == \
        ["vf_adam_set_scalars", "vf_grad_accum_multi"] * 2 + ["vf_adam_multi"], logged


def _micro_grads(dev, batch, A):
    """The raw gradient (and loss) of each of the A micro-batches, each run alone on a fresh identical model with the ids
    the undivided batch gives its samples."""
    vf = _model(dev)
    ids, n = _first_ids(dev), B // A
    out, losses = [], []
    for m in range(A):
        sl = slice(m * n, (m + 1) * n)
        vf.zero_grad()
        loss = vf(y_cond=batch["y_cond"][sl], view_count=batch["view_count"][sl], angle=batch["angle"][sl],
                  y_0=batch["y_0"][sl], seed=SEED, sample_ids=ids[sl])
        loss.backward()
        out.append(_grads(vf))
        losses.append(loss.detach())
    return out, losses


def test_accumulated_gradient_and_step_are_exact(dev):
    from view_fusion_amd.optim import FusedAdam
    batch = _batch(dev)
    micro, losses = _micro_grads(dev, batch, 2)
    want = accum_ref.accumulate_all(micro, [0.5, 0.5])
    vf, tr = _trainer(dev, False, accum_steps=2)
    loss = tr.step(batch)
    got = _grads(vf)
    assert len(got) == len(want) > 10
    for (k, _), a, b in zip(vf.named_parameters(), got, want):
        assert np.array_equal(_bits(a), _bits(b)), k
    assert any(not np.array_equal(_bits(a), _bits(m0)) for a, m0 in zip(got, micro[0]))     # (both halves count)
    assert torch.equal(loss, losses[0] * 0.5 + losses[1] * 0.5)
    # the parameters: FusedAdam's own step on that gradient, from the same start
    ref = _model(dev)
    opt = FusedAdam(list(ref.parameters()), lr=tr.opt.param_groups[0]["lr"])
    for p, g in zip(ref.parameters(), want):
        p.grad = torch.from_numpy(g).to(dev).reshape(p.shape)
    opt.step()
    torch.cuda.synchronize()
    for (k, p), q in zip(vf.named_parameters(), ref.parameters()):
        assert torch.equal(p, q), k
    assert tr.it == 1 and float(tr.opt.state_dict()["state"][0]["step"]) == 1.0


@pytest.fixture(scope="module")
def big_batch(dev):
    """The undivided batch (A = 1, the parent's path): its GPU gradient and loss, and the CPU oracle's for the same
    inputs -- the very draws the GPU used -- in float64.  Computed once; nothing below changes it."""
    from oracle import unet_ref, view_fusion_ref as vfr
    from view_fusion_amd import ops
    batch = _batch(dev)
    vf, tr = _trainer(dev, False)
    loss = float(tr.step(batch))
    names, g1 = [k for k, _ in vf.named_parameters()], _grads(vf)
    fresh = _model(dev)
    ids = _first_ids(dev)
    t, _, u = ops.draw_train(SEED, ids, fresh.gammas, want_u=True)
    noise = ops.randn_ids(SEED, ids, ops.diffusion.RNG_TRAIN_NOISE, 0, (3, HW, HW))
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in fresh.denoise_fn.state_dict().items()}
    buf = {k: v.double() for k, v in vfr.schedule_buffers(vfr.beta_schedule(**SCHED)).items()}
    assert torch.equal(buf["gammas"].float(), fresh.gammas.cpu())
    ref = vfr.train_loss(lambda x, a, l: unet_ref.unet_forward(sd, TINY, x, a, l), buf, batch["y_cond"].cpu().double(),
                         batch["view_count"], batch["angle"].cpu().double(), batch["y_0"].cpu().double(), t.cpu(),
                         u.cpu().double().reshape(-1, 1), noise.cpu().double(), True)
    ref.backward()
    g64 = [sd[k[len("denoise_fn."):]].grad.numpy() for k in names]
    e = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(g1, g64)]
    return dict(batch=batch, names=names, g1=g1, loss=loss, e=e, e_loss=abs(loss - float(ref)), loss64=float(ref))


@pytest.mark.parametrize("A", [2, 4])
def test_accumulated_gradient_matches_the_undivided_batch(dev, big_batch, A):
    r = big_batch
    vf, tr = _trainer(dev, False, accum_steps=A)
    loss = float(tr.step(r["batch"]))
    worst = (0.0, None)
    for k, g, g1, e in zip(r["names"], _grads(vf), r["g1"], r["e"]):
        diff, bound = float(np.abs(g.astype(np.float64) - g1).max()), 4.0 * e + 1e-7 * float(np.abs(g1).max())
        worst = max(worst, (diff / bound, k))
        print(f"A={A} {k:60s} max|g| {np.abs(g1).max():.3e}  e {e:.3e}  |g_A - g_1| {diff:.3e}  bound {bound:.3e}")
    bound = 4.0 * r["e_loss"] + 1e-7 * abs(r["loss"])
    print(f"A={A} loss {loss:.9g}  A=1 {r['loss']:.9g}  oracle f64 {r['loss64']:.12g}  e {r['e_loss']:.3e}  "
          f"|diff| {abs(loss - r['loss']):.3e}  bound {bound:.3e};  worst gradient diff / bound {worst[0]:.3f} ({worst[1]})")
    for k, g, g1, e in zip(r["names"], _grads(vf), r["g1"], r["e"]):
        assert float(np.abs(g.astype(np.float64) - g1).max()) <= 4.0 * e + 1e-7 * float(np.abs(g1).max()), k
    assert abs(loss - r["loss"]) <= bound


def _snapshot(vf, tr):
    torch.cuda.synchronize()
    sd = tr.opt.state_dict()["state"]
    n = len(list(vf.parameters()))
    out = dict(p=_params(vf), m=[sd[i]["exp_avg"].cpu().clone() for i in range(n)],
               v=[sd[i]["exp_avg_sq"].cpu().clone() for i in range(n)], g=[p.grad.cpu().clone() for p in vf.parameters()])
    if tr.opt.ema_decay is not None:
        out["ema"] = [tr.ema_state_dict()["state"][i].cpu().clone() for i in range(n)]
    return out


@pytest.mark.parametrize("extras", [False, True])
def test_graph_replay_equals_eager(dev, extras):
    kw = dict(ema_decay=0.9, max_grad_norm=0.05) if extras else {}
    (vf_e, tr_e), (vf_g, tr_g) = _trainer(dev, False, accum_steps=2, **kw), _trainer(dev, True, accum_steps=2, **kw)
    for s in range(3):
        le, lg = tr_e.step(_batch(dev, s)), tr_g.step(_batch(dev, s))
        assert torch.equal(le, lg), s
        if extras:
            assert float(tr_e.grad_norm) == float(tr_g.grad_norm) > 0.05, s
    # both micro-batches stack 4 views: one geometry, captured after two sightings (= the first step), 4 replays
    assert tr_e.graph_steps == 0 and tr_g.graph_steps == 4 and len(tr_g._graphs) == 1 and tr_g.mode == "graph"
    a, b = _snapshot(vf_e, tr_e), _snapshot(vf_g, tr_g)
    for k in a:
        assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k
    assert tr_e.it == tr_g.it == 3
    for tr in (tr_e, tr_g):
        assert float(tr.opt.state_dict()["state"][0]["step"]) == 3.0
        assert not extras or tr.ema_state_dict()["num_updates"] == 3


def test_clipping_and_ema_act_on_the_accumulated_gradient(dev, big_batch):
    norm1 = float(np.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in big_batch["g1"])))
    mx = 0.5 * norm1                                   # half the undivided batch's norm: the clip is active
    vf, tr = _trainer(dev, False, accum_steps=2, max_grad_norm=mx, ema_decay=0.9)
    start = [p.numpy().reshape(-1) for p in _params(vf)]
    tr.step(big_batch["batch"])
    torch.cuda.synchronize()
    gs = [g.reshape(-1) for g in _grads(vf)]           # the accumulated gradient (left raw in p.grad)
    ref = float(np.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in gs)))
    got = float(tr.grad_norm)
    e = abs(float(optim_ref.norm_scale_f32(gs, None)[0]) - ref) / ref
    print(f"grad_norm {got:.9g}  accumulated gradient's norm (double) {ref:.9g}  err {abs(got - ref) / ref:.3e}  "
          f"fp32 restatement e {e:.3e}  bound {optim_ref.bound(e):.3e}  max_grad_norm {mx:.4g}")
    assert abs(got - ref) / ref <= optim_ref.bound(e) and got > mx
    lr = tr.opt.param_groups[0]["lr"]
    kw = dict(lr=lr, max_norm=mx, ema_decay=0.9)
    r64 = optim_ref.run_f64(start, [gs], moment_betas=optim_ref.float_betas(), **kw)
    r32 = optim_ref.run_f32(start, [gs], **kw)
    assert r64["scale"][0] < 1.0
    snap = _snapshot(vf, tr)
    for key in ("p", "m", "v", "ema"):
        worst = 0.0
        for i, t in enumerate(snap[key]):
            x = t.numpy().reshape(-1)
            e, err = optim_ref.rel_err(r32[key][i], r64[key][i]), optim_ref.rel_err(x, r64[key][i])
            worst = max(worst, err / optim_ref.bound(e))
            assert err <= optim_ref.bound(e), (key, i, err, e)
        print(f"{key:3s}: worst err / bound over {len(snap[key])} tensors {worst:.3f}")
    assert tr.ema_state_dict()["num_updates"] == 1 and float(tr.opt.state_dict()["state"][0]["step"]) == 1.0
    tr.step(_batch(dev, 1))
    assert tr.ema_state_dict()["num_updates"] == 2 and float(tr.opt.state_dict()["state"][0]["step"]) == 2.0 and tr.it == 2
