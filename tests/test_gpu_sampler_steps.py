"""Few-step sampling on the GPU: the table-driven tail (vf_sampler_step / vf_sampler_step_rng) against the float64
restatement of tests/sampler_ref.py, generate(sample_steps=) at full length against the ancestral sampler, K-step chains
against the restatement through the oracle UNet, graph replay, the launches each path logs, batch invariance, drivers.

TINY 16 x 16, SCHED_C1 (T = 10), B = 3 with ragged view counts (1, 3, 2).
Tolerances: one kernel rel 2e-5 (max|a-b| / max|b|), chains max-abs 1e-3; "bitwise" is torch.equal."""
import numpy as np
import pytest
import torch

import sampler_ref
from conftest import SCHED_C1, TINY

pytestmark = pytest.mark.gpu
KERNEL_RTOL, CHAIN_TOL = 2e-5, 1e-3
HW = TINY["image_size"]
T = SCHED_C1["num_timesteps"]
VC = [1, 3, 2]
SOLVERS = [("ddim", 0.0), ("ddim", 0.5), ("ddim", 1.0), ("dpmpp2m", 0.0)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def vf(dev):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    m = ViewFusion(net.to(dev), {"train": SCHED_C1})
    m.set_new_noise_schedule(device=dev, phase="train")
    return m


@pytest.fixture(scope="module")
def case(vf, dev):
    """Inputs, injected draws and the oracle, computed once and left unchanged."""
    from oracle import unet_ref, view_fusion_ref as vfr
    g = torch.Generator().manual_seed(910)
    c = dict(y_cond=torch.rand(3, 3, 3, HW, HW, generator=g), angle=2 * np.pi / 24 * torch.randint(0, 24, (3, 1), generator=g).float(),
             y_T=torch.randn(3, 3, HW, HW, generator=g), z_seq=torch.randn(T, 3, 3, HW, HW, generator=g), vc=torch.tensor(VC))
    sd = {k: v.detach().cpu().clone() for k, v in vf.denoise_fn.state_dict().items()}
    c["betas"] = vfr.beta_schedule(**SCHED_C1)
    c["gammas32"] = vfr.schedule_buffers(c["betas"])["gammas"]
    c["unet"] = lambda x, a, l: unet_ref.unet_forward(sd, TINY, x, a, l)
    c["compose"] = vfr.compose
    c["gpu"] = {k: c[k].to(dev) for k in ("y_cond", "angle", "y_T", "z_seq")}
    return c


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _gen(vf, case, **kw):
    g = case["gpu"]
    return vf.generate(g["y_cond"], case["vc"], g["angle"], **kw)


def _ref_chain(case, K, solver, eta, z_seq=None, y_T=None):
    tau = sampler_ref.timesteps(T, K)
    with torch.no_grad():
        return sampler_ref.chain(case["unet"], case["compose"], case["betas"], case["gammas32"], tau, solver, eta,
                                 case["y_cond"], case["vc"], case["angle"], case["y_T"] if y_T is None else y_T, z_seq)


# ---- 1. one step against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("solver,eta", SOLVERS)
@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("H,W", [(16, 16), (4, 5)])       # 4 x 5: 15 float4 per sample, less than one workgroup
def test_step_against_the_restatement(vf, dev, H, W, weighting, solver, eta):
    from oracle import view_fusion_ref as vfr
    from view_fusion_amd import ops, schedule
    K, B = 5, 3
    betas = vfr.beta_schedule(**SCHED_C1)
    tau = schedule.sample_timesteps(T, K)
    plan = vf._sampler_plan(tau.tolist(), solver, eta, dev)
    g = torch.Generator().manual_seed(17 + H)
    out = torch.randn(sum(VC), 6, H, W, generator=g) * 2
    y, z, prev = (torch.randn(B, 3, H, W, generator=g) for _ in range(3))
    off, S, max_v = ops.view_offsets(VC, dev)
    eps, _, w_ref = vfr.compose(out, VC, weighting)
    nan = torch.full((B, 3, H, W), float("nan"))
    for k in range(K):
        second = solver == "dpmpp2m" and 0 < k < K - 1
        hist0 = prev if second else nan                    # before a first-order step the history may hold anything
        want, want_y0 = sampler_ref.step(betas, tau, solver, eta, k, y.double().numpy(), eps.double().numpy(),
                                         hist0.double().numpy(), z.double().numpy())
        kidx = torch.full((B,), k, device=dev)
        hist = hist0.to(dev)
        got, w = ops.sampler_step(out.to(dev), off, y.to(dev), z.to(dev), kidx, plan, B, max_v, weighting, y0_prev=hist)
        e, e0 = rel(got, want), rel(hist, want_y0)
        print(f"{solver} eta {eta} {H}x{W} weighting {weighting} k {k}: y_new rel {e:.2e}  y0 rel {e0:.2e}")
        assert torch.isfinite(got).all() and e <= KERNEL_RTOL and e0 <= KERNEL_RTOL
        # the weights are the ancestral tail's, bit for bit
        t = torch.full((B,), int(tau[k]), device=dev)
        _, _, w_tail = ops.p_sample_tail(out.to(dev), off, y.to(dev), z.to(dev), t, vf._sched(), B, max_v, weighting)
        if weighting:
            assert torch.equal(w, w_tail) and rel(w, w_ref) <= KERNEL_RTOL
        else:
            assert w is None and w_tail is None
        # in place = out of place, bit for bit; without a history buffer the same y_new where there is no c1
        y_in, hist_in = y.to(dev), hist0.to(dev)
        r_in, _ = ops.sampler_step(out.to(dev), off, y_in, z.to(dev), kidx, plan, B, max_v, weighting, y0_prev=hist_in,
                                   inplace=True, want_weights=False)
        assert r_in is y_in and torch.equal(y_in, got) and torch.equal(hist_in, hist)
        if not second:
            r_nh, _ = ops.sampler_step(out.to(dev), off, y.to(dev), z.to(dev), kidx, plan, B, max_v, weighting)
            assert torch.equal(r_nh, got)
    with pytest.raises(ValueError):
        ops.sampler_step(out.to(dev), off, y.to(dev), z.to(dev), kidx, plan, B, max_v, weighting, seed=1)


def test_step_draws_its_own_z_at_the_model_timestep(vf, dev):
    """vf_sampler_step_rng = vf_sampler_step fed with the normals of (seed, id, kind 3, step tau[k]); per-sample k."""
    from view_fusion_amd import ops, schedule
    B, seed, ids = 3, 0xC0FFEE, [4, 2 ** 33 + 1, 9]
    tau = schedule.sample_timesteps(T, 5).tolist()
    plan = vf._sampler_plan(tau, "ddim", 0.5, dev)
    g = torch.Generator().manual_seed(3)
    out, y = torch.randn(sum(VC), 6, HW, HW, generator=g).to(dev), torch.randn(B, 3, HW, HW, generator=g).to(dev)
    off, S, max_v = ops.view_offsets(VC, dev)
    ks = [4, 2, 0]                                          # sigma[0] == 0: that sample gets no noise at all
    kidx = torch.tensor(ks, device=dev)
    idt = torch.tensor(ids, dtype=torch.int64, device=dev)
    got, _ = ops.sampler_step(out, off, y, None, kidx, plan, B, max_v, True, seed=seed, ids=idt)
    z = torch.stack([ops.randn_ids(seed, idt[b:b + 1], ops.diffusion.RNG_STEP_NOISE, tau[k], (3, HW, HW))[0]
                     for b, k in enumerate(ks)])
    want, _ = ops.sampler_step(out, off, y, z, kidx, plan, B, max_v, True)
    quiet, _ = ops.sampler_step(out, off, y, None, kidx, plan, B, max_v, True)
    assert torch.equal(got, want) and torch.equal(got[2], quiet[2]) and not torch.equal(got[0], quiet[0])


# ---- 2. full length = the ancestral sampler -------------------------------------------------------------------------
def test_full_length_ddim_eta1_equals_the_ancestral_chain(vf, case):
    g = case["gpu"]
    a = _gen(vf, case, y_t=g["y_T"], z_seq=g["z_seq"])
    b = _gen(vf, case, y_t=g["y_T"], z_seq=g["z_seq"], sample_steps=T, solver="ddim", eta=1.0)
    assert [tuple(x.shape) for x in a] == [tuple(x.shape) for x in b]
    err, werr = float((a[1] - b[1]).abs().max()), float((a[3] - b[3]).abs().max())
    print(f"sample_steps = T, ddim eta 1 vs default, injected draws: chain max-abs {err:.3e}  weights {werr:.3e}")
    assert err <= CHAIN_TOL and werr <= CHAIN_TOL and torch.equal(a[1][:, 0], b[1][:, 0])
    c = _gen(vf, case, seed=77, sample_ids=[5, 9, 2 ** 34])
    d = _gen(vf, case, seed=77, sample_ids=[5, 9, 2 ** 34], sample_steps=T, solver="ddim", eta=1.0)
    err = float((c[1] - d[1]).abs().max())
    print(f"the same, seeded and nothing injected: chain max-abs {err:.3e}")
    assert err <= CHAIN_TOL and torch.equal(c[1][:, 0], d[1][:, 0])
    assert float((c[4] - a[4]).abs().max()) > 10 * CHAIN_TOL          # (and the two pairs are different samples)


# ---- 3. K-step chains against the restatement through the oracle UNet ---------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 5])
@pytest.mark.parametrize("solver,eta", [("ddim", 0.0), ("ddim", 0.5), ("dpmpp2m", 0.0)])
def test_chain_against_the_oracle(vf, case, K, solver, eta):
    g = case["gpu"]
    y, ret, logits, weights, samples = _gen(vf, case, y_t=g["y_T"], z_seq=g["z_seq"] if eta else None, sample_steps=K,
                                            solver=solver, eta=eta)
    states, w_ref = _ref_chain(case, K, solver, eta, z_seq=case["z_seq"] if eta else None)
    every = max(1, K // 8)
    keep = [i for i, k in enumerate(reversed(range(K))) if k % every == 0]
    assert ret.shape == (3, 1 + len(keep), 3, HW, HW) and weights.shape == (3, len(keep), 3, 3, HW, HW)
    assert logits.shape == (sum(VC), len(keep), 3, HW, HW)
    err = float((ret[:, 1:].cpu() - states[keep].transpose(0, 1)).abs().max())
    werr = float((weights.cpu() - torch.stack([w_ref[i] for i in keep], dim=1)).abs().max())
    print(f"{solver} eta {eta} K {K}: chain max-abs {err:.3e}  weights {werr:.3e}")
    assert torch.equal(ret[:, 0], g["y_T"]) and torch.equal(samples, ret[:, -1]) and torch.equal(y, samples)
    assert err <= CHAIN_TOL and werr <= CHAIN_TOL
    assert samples.abs().max() <= 1.0                                   # the last step lands on the clamped y0


def test_explicit_timesteps_and_snapshots(vf, case):
    """An explicit sequence is a chain of its own; sample_num picks the snapshots k % (K // sample_num) == 0."""
    g = case["gpu"]
    tau = [1, 4, 6, 9]
    _, ret, _, weights, _ = _gen(vf, case, y_t=g["y_T"], sample_steps=tau, solver="dpmpp2m", sample_num=2)
    with torch.no_grad():
        states, _ = sampler_ref.chain(case["unet"], case["compose"], case["betas"], case["gammas32"], np.array(tau),
                                      "dpmpp2m", 0.0, case["y_cond"], case["vc"], case["angle"], case["y_T"], None)
    assert ret.shape[1] == 3 and weights.shape[1] == 2                   # y_T, then k = 2 and k = 0
    err = float((ret[:, 1:].cpu() - states[[1, 3]].transpose(0, 1)).abs().max())
    print(f"dpmpp2m over tau {tau}: chain max-abs {err:.3e}")
    assert err <= CHAIN_TOL


def test_dpmpp2m_at_two_steps_is_ddim_eta0_bitwise(vf, case, dev):
    """Both steps are first order and the two solvers' tables differ only in float64 rounding: they round to the same
    fp32 on this schedule (asserted here, and on every schedule by test_sampler_host), so the chains are the same bits."""
    tau = sampler_ref.timesteps(T, 2).tolist()
    pa = {k: v.clone() for k, v in vf._sampler_plan(tau, "dpmpp2m", 0.0, dev).items() if torch.is_tensor(v)}
    pb = vf._sampler_plan(tau, "ddim", 0.0, dev)
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    g = case["gpu"]
    a = _gen(vf, case, y_t=g["y_T"], sample_steps=2, solver="dpmpp2m")
    b = _gen(vf, case, y_t=g["y_T"], sample_steps=2, solver="ddim", eta=0.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 4. graph replay, and what each path launches -------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(solver="ddim", eta=0.5, seed=8, sample_ids=[100, 200, 300]), dict(solver="dpmpp2m")],
                         ids=["ddim-seeded", "dpmpp2m"])
def test_graph_replay_equals_eager_bitwise(vf, case, kw):
    g = case["gpu"]
    if "seed" not in kw:
        kw = dict(kw, y_t=g["y_T"])
    a = _gen(vf, case, sample_steps=5, use_graph=True, **kw)
    b = _gen(vf, case, sample_steps=5, use_graph=False, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.isfinite(a[1]).all()


def test_launches_of_each_path(vf, case):
    from view_fusion_amd import ops

    def names(**kw):
        try:
            ops.st.KERNEL_LOG = []
            _gen(vf, case, use_graph=False, **kw)
            return [e[5] for e in ops.st.KERNEL_LOG]
        finally:
            ops.st.KERNEL_LOG = None

    new = {"vf_sampler_step", "vf_sampler_step_rng"}
    rng_state = torch.cuda.get_rng_state(case["gpu"]["y_T"].device)
    for solver in ("ddim", "dpmpp2m"):                                  # eta = 0: no z, loaded or drawn
        quiet = names(sample_steps=3, solver=solver, y_t=case["gpu"]["y_T"])
        assert quiet.count("vf_sampler_step") == 3 and not any(n.endswith("_rng") or n == "vf_randn_ids" for n in quiet)
        assert "vf_p_sample_tail" not in quiet
        seeded = names(sample_steps=3, solver=solver, seed=5)           # the seed only draws y_T
        assert seeded.count("vf_sampler_step") == 3 and seeded.count("vf_randn_ids") == 1
        assert not any(n.endswith("_rng") for n in seeded)
    assert torch.equal(torch.cuda.get_rng_state(case["gpu"]["y_T"].device), rng_state)
    noisy = names(sample_steps=3, eta=0.5, seed=5)
    assert noisy.count("vf_sampler_step_rng") == 3 and "vf_sampler_step" not in noisy
    loaded = names(sample_steps=3, eta=0.5, y_t=case["gpu"]["y_T"], z_seq=case["gpu"]["z_seq"])
    assert loaded.count("vf_sampler_step") == 3 and "vf_sampler_step_rng" not in loaded
    # the default call is the ancestral sampler, as before
    plain = names(y_t=case["gpu"]["y_T"], z_seq=case["gpu"]["z_seq"])
    assert plain.count("vf_p_sample_tail") == T and not (new & set(plain))
    plain_seeded = names(seed=5)
    assert not (new & set(plain_seeded)) and plain_seeded.count("vf_p_sample_tail_rng") == T


# ---- 5. batch invariance ----------------------------------------------------------------------------------------------
def test_few_step_sampling_does_not_depend_on_the_batch(vf, case, dev):
    g = case["gpu"]
    kw = dict(seed=31337, sample_steps=3, solver="ddim", eta=1.0)
    rng_state = torch.cuda.get_rng_state(dev)
    _, both, *_ = vf.generate(g["y_cond"][1:], case["vc"][1:], g["angle"][1:], sample_ids=[5, 9], **kw)
    for row, sid in ((0, 5), (1, 9)):
        _, one, *_ = vf.generate(g["y_cond"][1 + row:2 + row], case["vc"][1 + row:2 + row], g["angle"][1 + row:2 + row],
                                 sample_ids=torch.tensor([sid], device=dev), **kw)
        assert torch.equal(both[row, 0], one[0, 0])                       # y_T bitwise
        err = float((both[row] - one[0]).abs().max())
        print(f"id {sid} alone vs in a ragged batch of two: max-abs {err:.3e}")
        assert err <= CHAIN_TOL
    assert torch.equal(torch.cuda.get_rng_state(dev), rng_state)          # torch's device generator was not touched
    _, other, *_ = vf.generate(g["y_cond"][2:3], case["vc"][2:3], g["angle"][2:3], sample_ids=[8], **kw)
    assert float((other - one).abs().max()) > 10 * CHAIN_TOL              # another id: another sample


# ---- 6. drivers ---------------------------------------------------------------------------------------------------------
def test_drivers_pass_the_sampler_through(vf, dev):
    from view_fusion_amd import drivers
    g = torch.Generator().manual_seed(700)
    full = dict(target=torch.rand(4, 3, HW, HW, generator=g).to(dev), cond=torch.rand(4, 6, 3, HW, HW, generator=g).to(dev),
                angle=torch.rand(4, 1, generator=g).to(dev), view_count=torch.tensor([2, 6, 3, 1]),
                ids=torch.tensor([11, 5, 2 ** 33, 8]))
    halves = [{k: v[lo:hi] for k, v in full.items()} for lo, hi in ((0, 2), (2, 4))]
    got = {}

    def keep(tag):
        got[tag] = []
        return {"keep": lambda a, t: (got[tag].append(a.clone()), a.flatten(1).mean(1))[1]}

    one = drivers.evaluate(vf, [full], seed=21, ssim=True, sample_steps=3, extra_metrics=keep("one"))
    two = drivers.evaluate(vf, halves, seed=21, ssim=True, sample_steps=3, extra_metrics=keep("two"))
    assert all(torch.isfinite(v) for v in one.values()) and set(one) == {"psnr", "ssim", "keep"}
    a, b = torch.cat(got["one"]), torch.cat(got["two"])
    err = float((a - b).abs().max())
    print(f"evaluate(sample_steps=3): one batch of four vs two of two: samples max-abs {err:.3e}  psnr "
          f"{float(one['psnr']):.5f} / {float(two['psnr']):.5f}")
    assert a.shape == (4, 3, HW, HW) and err <= CHAIN_TOL
    _ = drivers.evaluate(vf, [full], seed=21, extra_metrics=keep("full"))
    assert float((torch.cat(got["full"]) - a).abs().max()) > 10 * CHAIN_TOL       # three steps are not ten
    first = torch.rand(2, 3, HW, HW, generator=g).to(dev)
    r = drivers.autoregressive_rollout(vf, first, steps=2, sample_steps=2, seed=4)
    assert r.shape == (2, 2, 3, HW, HW) and torch.isfinite(r).all()
    assert torch.equal(r, drivers.autoregressive_rollout(vf, first, steps=2, sample_steps=2, solver="dpmpp2m", seed=4))
    assert not torch.equal(r, drivers.autoregressive_rollout(vf, first, steps=2, seed=4))
