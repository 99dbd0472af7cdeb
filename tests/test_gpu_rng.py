"""The seeded counter-based draws (csrc/rng.h) on the GPU, all through the C ABI: device against the host mirrors and the
numpy restatement (tests/rng_ref.py), batch invariance of training and sampling, the DEFAULT-shaped paths (nothing
injected on the GPU side) against the CPU oracle fed with draws that rng_ref computes, graph replay, evaluate().

Tolerances: integers, uniforms and raw words bit-equal; normals within rng_ref.bound (max(4 e, 1e-6), e = the float32
restatement's own error on the same counters); chains max-abs 1e-3 and losses rel 1e-5."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import rng_ref
from conftest import SCHED_C1, TINY

pytestmark = pytest.mark.gpu
CHAIN_TOL, LOSS_RTOL = 1e-3, 1e-5          # stated chain / loss tolerances
HW = TINY["image_size"]
N_IMG = 3 * HW * HW
IDS = [0, 1, 2, 1000, 2 ** 32 - 1, 2 ** 32, 2 ** 40 - 1, 2 ** 40]
SEEDS = [0, 0xDEADBEEFCAFEF00D]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ids(ids, dev):
    return torch.tensor(ids, dtype=torch.int64, device=dev)


def _model(dev, sched=SCHED_C1):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": sched})
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


def _inputs(B, N, seed=500):
    g = torch.Generator().manual_seed(seed)
    return dict(y_0=torch.rand(B, 3, HW, HW, generator=g), y_cond=torch.rand(B, N, 3, HW, HW, generator=g),
                angle=2 * np.pi / 24 * torch.randint(0, 24, (B, 1), generator=g).float())


def _oracle(vf):
    from oracle import unet_ref, view_fusion_ref as vfr
    sd = {k: v.detach().cpu().clone() for k, v in vf.denoise_fn.state_dict().items()}
    buf = vfr.schedule_buffers(vfr.beta_schedule(**SCHED_C1))
    return vfr, buf, (lambda x, a, l: unet_ref.unet_forward(sd, TINY, x, a, l))


def _ref_chain_draws(seed, ids, T):
    """y_T and z_seq of generate(seed=) as rng_ref states them (float64 restatement, rounded to fp32 once)."""
    B = len(ids)
    y_T = torch.tensor(rng_ref.normal(seed, ids, rng_ref.KIND_START_NOISE, 0, N_IMG)).float().reshape(B, 3, HW, HW)
    z = [torch.zeros(B, 3, HW, HW)]
    z += [torch.tensor(rng_ref.normal(seed, ids, rng_ref.KIND_STEP_NOISE, i, N_IMG)).float().reshape(B, 3, HW, HW)
          for i in range(1, T)]
    return y_T, torch.stack(z)


# ---- device against host ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_words_integers_and_uniforms_are_bit_equal(dev, seed):
    from view_fusion_amd import _lib, ops
    lib = _lib.load()
    ids = IDS + list(range(7000, 7100))
    for kind, step in [(1, 0), (3, 999), (3, 2 ** 28 - 1)]:
        w = ops.philox_ids(seed, _ids(ids, dev), kind, step, 64).cpu().numpy().view(np.uint32)
        assert np.array_equal(w.astype(np.uint64), rng_ref.words(seed, ids, kind, step, 16).reshape(len(ids), 64))
    # a few counters through the host mirror of the Philox call itself
    w = ops.philox_ids(seed, _ids(IDS, dev), 2, 0, 8).cpu().numpy().view(np.uint32)
    for r, i in enumerate(IDS):
        for blk in range(2):
            c = np.array([blk, i & 0xFFFFFFFF, i >> 32, 2 << 28], dtype=np.uint32)
            k = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
            o = np.zeros(4, dtype=np.uint32)
            assert lib.vf_rng_host_philox(ctypes.c_void_p(c.ctypes.data), ctypes.c_void_p(k.ctypes.data),
                                          ctypes.c_void_p(o.ctypes.data)) == 0
            assert np.array_equal(w[r, 4 * blk:4 * blk + 4], o)
    for T in (2, 10, 1000, 2000):
        gam = torch.linspace(0.999, 0.001, T, device=dev)
        t, level, u = ops.draw_train(seed, _ids(ids, dev), gam, want_u=True)
        assert t.dtype == torch.int64 and u.dtype == torch.float32
        a = np.ascontiguousarray(ids, dtype=np.int64)
        th, uh = np.empty(len(ids), dtype=np.int64), np.empty(len(ids), dtype=np.float32)
        assert lib.vf_rng_host_train_scalars(seed, ctypes.c_void_p(a.ctypes.data), T, ctypes.c_void_p(th.ctypes.data),
                                             ctypes.c_void_p(uh.ctypes.data), len(ids)) == 0
        tr, ur = rng_ref.train_scalars(seed, ids, T)
        assert np.array_equal(t.cpu().numpy(), th) and np.array_equal(th, tr)
        assert np.array_equal(u.cpu().numpy().view(np.uint32), uh.view(np.uint32)) and np.array_equal(uh, ur)
        assert int(t.min()) >= 1 and int(t.max()) <= T - 1 and float(u.min()) >= 0 and float(u.max()) < 1
        g64 = gam.double().cpu().numpy()
        want = (g64[tr] - g64[tr - 1]) * ur.astype(np.float64) + g64[tr - 1]
        # three fp32 roundings of values <= 1 (the difference, the product-sum, and gammas are exact inputs)
        assert np.abs(level.double().cpu().numpy() - want).max() <= 3 * 2.0 ** -24
        assert torch.equal(level, ops.gather_level(gam, t, u))            # the unseeded kernel on the same draws


@pytest.mark.parametrize("kind,step", [(1, 0), (2, 0), (3, 1), (3, 999)])
@pytest.mark.parametrize("seed", SEEDS)
def test_normals_against_float64(dev, seed, kind, step):
    from view_fusion_amd import ops
    got = ops.randn_ids(seed, _ids(IDS, dev), kind, step, (3, HW, HW))
    assert got.shape == (len(IDS), 3, HW, HW) and got.dtype == torch.float32
    r64, e, bound = rng_ref.bound(seed, IDS, kind, step, N_IMG)
    err = float(np.abs(got.double().cpu().numpy().reshape(len(IDS), -1) - r64).max())
    print(f"seed {seed:#x} kind {kind} step {step}: e {e:.3e}  bound {bound:.3e}  |gpu - fp64| {err:.3e}")
    assert err <= bound, (err, bound)
    # layout independence on the device: two calls of two ids = one call of four, bitwise
    two = torch.cat([ops.randn_ids(seed, _ids(IDS[:2], dev), kind, step, (3, HW, HW)),
                     ops.randn_ids(seed, _ids(IDS[2:4], dev), kind, step, (3, HW, HW))])
    assert torch.equal(two, got[:4])


def test_tail_draws_its_own_z(dev):
    """z recovered as (y_next - mean) / sigma from vf_p_sample_tail_rng, on a schedule whose sigma is 1 (so the
    recovery adds one fp32 rounding of y_next, |y_next| < 8: 2.4e-7); exactly 0 where t == 0."""
    from view_fusion_amd import ops
    vf = _model(dev)
    seed, ids, vc = 0x5EED, [3, 2 ** 33 + 5, 11, 12], [2, 1, 3, 2]
    tt = [9, 4, 0, 1]
    g = torch.Generator().manual_seed(1)
    out = torch.randn(sum(vc), 6, HW, HW, generator=g).to(dev)
    y_t = torch.randn(4, 3, HW, HW, generator=g).to(dev)
    t = torch.tensor(tt, device=dev)
    off, S, max_v = ops.view_offsets(vc, dev)
    sched = dict(vf._sched(), posterior_log_variance_clipped=torch.zeros(10, device=dev))
    y_next, mean, w = ops.p_sample_tail(out, off, y_t, None, t, sched, 4, max_v, True, want_mean=True, seed=seed,
                                        ids=_ids(ids, dev))
    y0, mean0, w0 = ops.p_sample_tail(out, off, y_t, None, t, sched, 4, max_v, True, want_mean=True)
    assert torch.equal(mean, mean0) and torch.equal(w, w0)               # everything but z is the unseeded tail
    z = (y_next.double() - mean.double()).cpu().numpy().reshape(4, -1)
    assert torch.equal(y_next[2], mean[2]) and not z[2].any()            # t == 0: exactly zero
    for b in (0, 1, 3):
        r64, e, bound = rng_ref.bound(seed, [ids[b]], rng_ref.KIND_STEP_NOISE, tt[b], N_IMG)
        err = float(np.abs(z[b] - r64[0]).max())
        print(f"sample {b} t {tt[b]}: e {e:.3e}  bound {bound:.3e}  |z - fp64| {err:.3e}")
        assert err <= bound, (b, err, bound)
    # the loaded-z kernel on the device's own normals gives the same step
    zz = torch.stack([ops.randn_ids(seed, _ids([i], dev), 3, s, (3, HW, HW))[0] if s else torch.zeros(3, HW, HW, device=dev)
                      for i, s in zip(ids, tt)])
    assert torch.equal(ops.p_sample_tail(out, off, y_t, zz, t, sched, 4, max_v, True)[0], y_next)
    with pytest.raises(ValueError):
        ops.p_sample_tail(out, off, y_t, zz, t, sched, 4, max_v, True, seed=seed)


# ---- batch invariance ---------------------------------------------------------------------------------------------
def test_training_draws_do_not_depend_on_the_batch(dev):
    from view_fusion_amd import ops
    vf = _model(dev)
    seed, ids, vc = 77, [40, 41, 2 ** 35, 43], [3, 1, 2, 3]
    inp = {k: v.to(dev) for k, v in _inputs(4, 3).items()}
    full = ops.draw_train(seed, _ids(ids, dev), vf.gammas, want_u=True)
    nf = ops.randn_ids(seed, _ids(ids, dev), 1, 0, (3, HW, HW))
    for lo, hi in ((0, 2), (2, 4)):
        part = ops.draw_train(seed, _ids(ids[lo:hi], dev), vf.gammas, want_u=True)
        for a, b in zip(full, part):
            assert torch.equal(a[lo:hi], b)
        assert torch.equal(nf[lo:hi], ops.randn_ids(seed, _ids(ids[lo:hi], dev), 1, 0, (3, HW, HW)))
    # every view of a sample is noised with the sample's own noise (ragged view_count)
    off, S, _ = ops.view_offsets(vc, dev)
    x, _, _ = ops.stack_views(inp["y_cond"], inp["y_0"], nf, full[1], inp["angle"], off, S)
    o = np.cumsum([0] + vc)
    for b in range(4):
        want = full[1][b].sqrt() * inp["y_0"][b] + (1 - full[1][b]).sqrt() * nf[b]
        for v in range(o[b], o[b + 1]):
            assert torch.equal(x[v, 3:], x[o[b], 3:])
            assert float((x[v, 3:] - want).abs().max()) <= 1e-6
    # forward(seed=) uses exactly these draws, and the loss of the batch is the mean of its halves' losses
    kw = dict(seed=seed)
    with torch.no_grad():
        whole = vf(inp["y_cond"], torch.tensor(vc), inp["angle"], y_0=inp["y_0"], sample_ids=ids, **kw)
        same = vf(inp["y_cond"], torch.tensor(vc), inp["angle"], y_0=inp["y_0"], t=full[0], u=full[2], noise=nf)
        halves = [vf(inp["y_cond"][lo:hi], torch.tensor(vc[lo:hi]), inp["angle"][lo:hi], y_0=inp["y_0"][lo:hi],
                     sample_ids=_ids(ids[lo:hi], dev), **kw) for lo, hi in ((0, 2), (2, 4))]
        other = vf(inp["y_cond"], torch.tensor(vc), inp["angle"], y_0=inp["y_0"], sample_ids=[1, 2, 3, 4], **kw)
        # an injected draw wins on its own: noise injected, t / u still from the generator
        mixed = vf(inp["y_cond"], torch.tensor(vc), inp["angle"], y_0=inp["y_0"], sample_ids=ids, noise=nf, **kw)
    print(f"whole {float(whole):.8f}  injected {float(same):.8f}  halves {[float(h) for h in halves]}")
    assert torch.equal(whole, same) and torch.equal(whole, mixed)
    mean = 0.5 * (float(halves[0]) + float(halves[1]))
    assert abs(float(whole) - mean) <= LOSS_RTOL * abs(mean)
    assert abs(float(other) - float(whole)) > 1e-3 * abs(float(whole))


def test_sampling_does_not_depend_on_the_batch(dev):
    vf = _model(dev)
    seed = 31337
    inp = {k: v.to(dev) for k, v in _inputs(3, 3, seed=501).items()}
    vc = [2, 3, 1]
    rng_state = torch.cuda.get_rng_state(dev)
    _, ret3, *_ = vf.generate(inp["y_cond"], torch.tensor(vc), inp["angle"], seed=seed, sample_ids=[3, 7, 9])
    _, ret1, *_ = vf.generate(inp["y_cond"][1:2], torch.tensor(vc[1:2]), inp["angle"][1:2], seed=seed,
                              sample_ids=_ids([7], dev))
    assert torch.equal(torch.cuda.get_rng_state(dev), rng_state)          # torch's device generator was not touched
    assert torch.equal(ret3[1, 0], ret1[0, 0])                            # y_T bitwise
    err = float((ret3[1] - ret1[0]).abs().max())
    print(f"one object alone vs inside a ragged batch of three: max-abs {err:.3e}")
    assert err <= CHAIN_TOL
    _, ret_other, *_ = vf.generate(inp["y_cond"][1:2], torch.tensor(vc[1:2]), inp["angle"][1:2], seed=seed,
                                   sample_ids=[8])
    assert float((ret_other - ret1).abs().max()) > 10 * CHAIN_TOL          # another id: another sample


# ---- the default-shaped paths against the oracle, nothing injected on the GPU side -----------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_generate_against_the_oracle(dev, use_graph):
    vf = _model(dev)
    vfr, buf, fn = _oracle(vf)
    seed, ids, vc = 2024, [5, 2 ** 36 + 1], torch.tensor([3, 2])
    inp = _inputs(2, 3, seed=502)
    y, ret, logits, weights, samples = vf.generate(inp["y_cond"].to(dev), vc, inp["angle"].to(dev), seed=seed,
                                                   sample_ids=ids, use_graph=use_graph)
    y_T, z_seq = _ref_chain_draws(seed, ids, 10)
    with torch.no_grad():
        yr, retr, lr, wr, _ = vfr.generate(fn, buf, inp["y_cond"], vc, inp["angle"], y_T, z_seq)
    err, werr = float((ret.cpu() - retr).abs().max()), float((weights.cpu() - wr).abs().max())
    print(f"generate(seed=) vs oracle with rng_ref draws (graph={use_graph}): chain max-abs {err:.3e}  weights {werr:.3e}")
    assert err <= CHAIN_TOL and werr <= CHAIN_TOL
    r64, e, bound = rng_ref.bound(seed, ids, rng_ref.KIND_START_NOISE, 0, N_IMG)
    assert float(np.abs(ret[:, 0].double().cpu().numpy().reshape(2, -1) - r64).max()) <= bound      # y_T itself
    # the default ids are arange(B)
    _, ret_d, *_ = vf.generate(inp["y_cond"].to(dev), vc, inp["angle"].to(dev), seed=seed, use_graph=use_graph)
    _, ret_e, *_ = vf.generate(inp["y_cond"].to(dev), vc, inp["angle"].to(dev), seed=seed, sample_ids=[0, 1],
                               use_graph=use_graph)
    assert torch.equal(ret_d, ret_e)


def test_training_loss_against_the_oracle(dev):
    vf = _model(dev)
    vfr, buf, fn = _oracle(vf)
    seed, ids, vc = 99, [17, 18, 2 ** 34], torch.tensor([2, 3, 1])
    inp = _inputs(3, 3, seed=503)
    loss = vf(inp["y_cond"].to(dev), vc, inp["angle"].to(dev), y_0=inp["y_0"].to(dev), seed=seed, sample_ids=ids)
    t, u = rng_ref.train_scalars(seed, ids, 10)
    noise = torch.tensor(rng_ref.normal(seed, ids, rng_ref.KIND_TRAIN_NOISE, 0, N_IMG)).float().reshape(3, 3, HW, HW)
    with torch.no_grad():
        ref = vfr.train_loss(fn, buf, inp["y_cond"], vc, inp["angle"], inp["y_0"], torch.tensor(t),
                             torch.tensor(u).reshape(-1, 1), noise, True)
    print(f"forward(seed=) loss {float(loss):.8f}  oracle with rng_ref draws {float(ref):.8f}")
    assert abs(float(loss) - float(ref)) <= LOSS_RTOL * abs(float(ref))
    loss.backward()                                                       # the seeded forward trains
    assert all(p.grad is not None for p in vf.denoise_fn.parameters())


# ---- graphs ---------------------------------------------------------------------------------------------------
def test_generate_graph_equals_eager_bitwise(dev):
    vf = _model(dev)
    inp = {k: v.to(dev) for k, v in _inputs(2, 3, seed=504).items()}
    a = vf.generate(inp["y_cond"], torch.tensor([3, 2]), inp["angle"], seed=8, sample_ids=[100, 200], use_graph=True)
    b = vf.generate(inp["y_cond"], torch.tensor([3, 2]), inp["angle"], seed=8, sample_ids=[100, 200], use_graph=False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # an injected z_seq still wins over the seed (y_T then still comes from the seed)
    z_seq = torch.randn(10, 2, 3, HW, HW, generator=torch.Generator().manual_seed(3)).to(dev)
    c = vf.generate(inp["y_cond"], torch.tensor([3, 2]), inp["angle"], seed=8, sample_ids=[100, 200], z_seq=z_seq)
    d = vf.generate(inp["y_cond"], torch.tensor([3, 2]), inp["angle"], y_t=a[1][:, 0], z_seq=z_seq)
    assert torch.equal(c[1], d[1]) and not torch.equal(c[1], a[1])


def test_seeded_trainer_graph_equals_eager_bitwise():
    """Pattern of tests/test_gpu_step_graph.py: six iterations, parameters and losses bit for bit; the sample ids are a
    graph input that the Trainer rewrites before every step."""
    from view_fusion_amd import train
    ma = train.build_model(unet_params=TINY, device="cuda:0", seed=3)
    mb = copy.deepcopy(ma)
    ta = train.Trainer(ma, graph=False, lr_warmup=4, seed=1234)
    tb = train.Trainer(mb, graph=True, lr_warmup=4, seed=1234)
    batches = [train.synthetic_batch(2, 3, 16, device="cuda:0", seed=100 + i) for i in range(6)]
    rng_state = torch.cuda.get_rng_state("cuda:0")
    losses = []
    for i, bt in enumerate(batches):
        la, lb = ta.step(bt), tb.step(bt)
        assert torch.equal(la, lb), i
        for (k, p), q in zip(ma.named_parameters(), mb.parameters()):
            assert torch.equal(p, q), (i, k)
        losses.append(float(la))
    assert ta.graph_steps == 0 and tb.graph_steps == 6 - train.Trainer.GRAPH_AFTER
    assert torch.equal(torch.cuda.get_rng_state("cuda:0"), rng_state)     # no draw came from torch's generator
    assert len(set(losses)) == 6
    # iteration `it` drew for ids it * B + b: the same loss from a plain forward with those ids on a fresh copy
    mc = train.build_model(unet_params=TINY, device="cuda:0", seed=3)
    l0 = mc(y_cond=batches[0]["y_cond"], view_count=batches[0]["view_count"], angle=batches[0]["angle"],
            y_0=batches[0]["y_0"], seed=1234, sample_ids=[0, 1])
    assert abs(float(l0) - losses[0]) <= LOSS_RTOL * losses[0]
    # a different seed is a different run
    md = train.build_model(unet_params=TINY, device="cuda:0", seed=3)
    assert float(train.Trainer(md, graph=False, lr_warmup=4, seed=1235).step(batches[0])) != losses[0]


# ---- drivers ----------------------------------------------------------------------------------------------------
def _eval_batches(dev):
    g = torch.Generator().manual_seed(700)
    full = dict(target=torch.rand(4, 3, HW, HW, generator=g).to(dev), cond=torch.rand(4, 6, 3, HW, HW, generator=g).to(dev),
                angle=torch.rand(4, 1, generator=g).to(dev), view_count=torch.tensor([2, 6, 3, 1]),
                ids=torch.tensor([11, 5, 2 ** 33, 8]))
    halves = [{k: v[lo:hi] for k, v in full.items()} for lo, hi in ((0, 2), (2, 4))]
    return full, halves


def test_evaluate_is_independent_of_the_batching(dev):
    from view_fusion_amd import drivers
    vf = _model(dev)
    full, halves = _eval_batches(dev)
    got = {}

    def keep(tag):
        got[tag] = []
        return {"keep": lambda g, t: (got[tag].append(g.clone()), g.flatten(1).mean(1))[1]}

    one = drivers.evaluate(vf, [full], seed=21, ssim=True, extra_metrics=keep("one"))
    two = drivers.evaluate(vf, halves, seed=21, ssim=True, extra_metrics=keep("two"))
    a, b = torch.cat(got["one"]), torch.cat(got["two"])
    err = float((a - b).abs().max())
    print(f"evaluate(seed=): one batch of four vs two of two: samples max-abs {err:.3e}  psnr {float(one['psnr']):.5f} / "
          f"{float(two['psnr']):.5f}  ssim {float(one['ssim']):.6f} / {float(two['ssim']):.6f}")
    assert a.shape == (4, 3, HW, HW) and err <= CHAIN_TOL
    # without "ids": a running index over this rank's images, the same for either batching
    noid = [{k: v for k, v in h.items() if k != "ids"} for h in halves]
    drivers.evaluate(vf, noid, seed=21, extra_metrics=keep("run"))
    drivers.evaluate(vf, [dict(full, ids=torch.arange(4))], seed=21, extra_metrics=keep("ar"))
    assert float((torch.cat(got["run"]) - torch.cat(got["ar"])).abs().max()) <= CHAIN_TOL


def test_evaluate_unseeded_launches_no_seeded_kernel(dev):
    from view_fusion_amd import drivers, ops
    vf = _model(dev)
    full, _ = _eval_batches(dev)
    seeded = ("vf_p_sample_tail_rng", "vf_randn_ids", "vf_draw_train", "vf_philox_ids")
    try:
        ops.st.KERNEL_LOG = []
        drivers.evaluate(vf, [full], use_graph=False)
        plain = {e[5] for e in ops.st.KERNEL_LOG}
        ops.st.KERNEL_LOG = []
        drivers.evaluate(vf, [full], use_graph=False, seed=21)
        with_seed = {e[5] for e in ops.st.KERNEL_LOG}
    finally:
        ops.st.KERNEL_LOG = None
    assert "vf_p_sample_tail" in plain and not (set(seeded) & plain) and not any(n.endswith("_rng") for n in plain)
    assert {"vf_p_sample_tail_rng", "vf_randn_ids"} <= with_seed and "vf_p_sample_tail" not in with_seed


def test_rollout_seed_uses_the_count_in_the_id(dev):
    from view_fusion_amd import drivers
    vf = _model(dev)
    first = torch.rand(2, 3, HW, HW, generator=torch.Generator().manual_seed(9)).to(dev)
    a = drivers.autoregressive_rollout(vf, first, steps=2, seed=4)
    b = drivers.autoregressive_rollout(vf, first, steps=2, seed=4)
    assert a.shape == (2, 2, 3, HW, HW) and torch.equal(a, b)
    # object 1 alone under its own id: the same rollout within the chain tolerance
    c = drivers.autoregressive_rollout(vf, first[1:], steps=2, seed=4, sample_ids=[1])
    assert float((c[0] - a[1]).abs().max()) <= CHAIN_TOL
    # step `count` of object b starts from the y_T of id b * steps + count - 1
    cond = torch.cat((first[1:, None], a[1:, :1]), dim=1)
    *_, smp = vf.generate(cond, torch.tensor([2]), torch.full((1, 1), 2 * np.pi / 24 * 2, device=dev), seed=4,
                          sample_ids=[1 * 2 + 1])
    assert float((smp[0] - a[1, 1]).abs().max()) <= CHAIN_TOL
