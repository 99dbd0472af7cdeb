"""Dynamic thresholding and guidance rescaling on the GPU (the head of csrc/diffusion.hip holds the definition,
tests/threshold_ref.py restates it): the exact selection alone (ops.abs_quantile), the four tails on the eps buffer against
the float64 restatement and against the tails they replace, generate() against the restatement through the oracle UNet,
graph replay, independence of the batch, the public entry points and the launches each path logs.

TINY 16 x 16, SCHED_C1 (T = 10), B = 3 with ragged view counts (1, 3, 2) -- the fixtures and tolerances of
test_gpu_guidance.py: one kernel rel 2e-5 (max|a-b| / max|b|), chains max-abs chain_tol(g); "bitwise" is torch.equal."""
import numpy as np
import pytest
import torch

import sampler_ref
import threshold_ref
from conftest import SCHED_C1, TINY

pytestmark = pytest.mark.gpu
KERNEL_RTOL, CHAIN_TOL = 2e-5, 1e-3
HW = TINY["image_size"]
T = SCHED_C1["num_timesteps"]
VC = [1, 3, 2]
NEW = {"vf_compose_eps", "vf_sample_stat", "vf_abs_quantile", "vf_p_sample_tail_eps", "vf_p_sample_tail_eps_rng",
       "vf_sampler_step_eps", "vf_sampler_step_eps_rng"}
OLD_TAILS = {"vf_p_sample_tail", "vf_p_sample_tail_rng", "vf_sampler_step", "vf_sampler_step_rng", "vf_p_sample_tail_cfg",
             "vf_p_sample_tail_cfg_rng", "vf_sampler_step_cfg", "vf_sampler_step_cfg_rng"}


def chain_tol(g):
    return (g + abs(1.0 - g)) * CHAIN_TOL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dev):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    m = ViewFusion(net.to(dev), {"train": SCHED_C1})
    m.set_new_noise_schedule(device=dev, phase="train")
    return m


@pytest.fixture(scope="module")
def vf(dev):
    return _model(dev)


@pytest.fixture(scope="module")
def case(vf, dev):
    """Inputs, injected draws and the oracle, computed once and left unchanged."""
    from oracle import unet_ref, view_fusion_ref as vfr
    g = torch.Generator().manual_seed(911)
    c = dict(y_cond=torch.rand(3, 3, 3, HW, HW, generator=g), angle=2 * np.pi / 24 * torch.randint(0, 24, (3, 1), generator=g).float(),
             y_T=torch.randn(3, 3, HW, HW, generator=g), z_seq=torch.randn(T, 3, 3, HW, HW, generator=g), vc=torch.tensor(VC))
    sd = {k: v.detach().cpu().clone() for k, v in vf.denoise_fn.state_dict().items()}
    c["betas"] = vfr.beta_schedule(**SCHED_C1)
    c["unet"] = lambda x, a, l: unet_ref.unet_forward(sd, TINY, x, a, l)
    c["gpu"] = {k: c[k].to(dev) for k in ("y_cond", "angle", "y_T", "z_seq")}
    return c


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _gen(vf, case, **kw):
    g = case["gpu"]
    return vf.generate(g["y_cond"], case["vc"], g["angle"], **kw)


def _names(fn):
    from view_fusion_amd import ops
    try:
        ops.st.KERNEL_LOG = []
        fn()
        return [e[5] for e in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None


# ---- 1. the selection alone -------------------------------------------------------------------------------------------
def _rows(n):
    """Three rows of n values: (0) normals quantised to multiples of 1/8 -- many ties, both signs; (1) one repeated value
    (at n = 73728 more than 65 535 equal values in one bin); (2) 0, -0.0, denormals of both signs, negative and positive
    unquantised values."""
    g = torch.Generator().manual_seed(1000 + n)
    tied = torch.round(torch.randn(n, generator=g) * 8) / 8
    same = torch.full((n,), -0.3125)
    tiny = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 3e-39, -7e-39, 1.17549435e-38, -2.0 ** -126])
    mixed = torch.cat([tiny.repeat(n // 24), -torch.rand(n // 3, generator=g), torch.randn(n, generator=g)])[:n]
    assert mixed.numel() == n
    return torch.stack([tied, same, mixed[torch.randperm(n, generator=g)]])


@pytest.mark.parametrize("n", [60, 768, 2880, 73728])
def test_abs_quantile_selects_exactly(dev, n):
    from view_fusion_amd import ops
    x = _rows(n)
    xs = np.sort(np.abs(x.numpy().astype(np.float64)), axis=1)
    assert (x[2] == 0).any() and (x[2].abs() < 1.1754944e-38).sum() > 4 and (x[2] < 0).any() and len(np.unique(xs[0])) < n
    x_d = x.to(dev)
    qs = [0.5 / (n - 1), 0.5, 0.995, (n - 2 + 0.5) / (n - 1), (n - 2) / (n - 1), 1.0]
    seen = set()
    for q in qs:
        k, frac = ops.quantile_position(n, q)
        seen.add(k)
        got = ops.abs_quantile(x_d, q)
        again = ops.abs_quantile(x_d, q)
        assert torch.equal(got, again)                                      # the same bits on every call
        got = got.cpu().numpy().astype(np.float64)
        want = threshold_ref.abs_quantile(x.numpy(), q)
        k1 = min(k + 1, n - 1)
        err = np.abs(got - want)
        bound = 4 * 2.0 ** -24 * xs[:, k1]            # three fp32 roundings of magnitudes <= x[k+1], one to spare
        print(f"n {n} q {q:.6f} k {k} frac {frac:.4f}: err {err} bound {bound}")
        assert (err <= bound).all(), (n, q, got, want)
        exact = (xs[:, k] == xs[:, k1]) | (frac == 0.0)
        assert (got[exact] == xs[exact, k]).all(), (n, q, got, xs[:, k])
        assert got[1] == 0.3125
    assert {0, n - 2, n - 1} <= seen
    # one row alone gives its row of the batch
    assert torch.equal(ops.abs_quantile(x_d[2:], 0.995), ops.abs_quantile(x_d, 0.995)[2:])


def test_abs_quantile_sizes_around_the_workgroup(dev):
    """n = 1, below / at / just above one workgroup of 1024, not a multiple of 4: against the float64 sort."""
    from view_fusion_amd import ops
    g = torch.Generator().manual_seed(77)
    for n in (1, 2, 3, 63, 1023, 1024, 1025, 4099):
        x = torch.randn(2, n, generator=g)
        for q in (0.0, 0.3, 0.995, 1.0):
            got = ops.abs_quantile(x.to(dev), q).cpu().numpy().astype(np.float64)
            want = threshold_ref.abs_quantile(x.numpy(), q)
            assert (np.abs(got - want) <= 4 * 2.0 ** -24 * np.abs(x.numpy()).max(axis=1)).all(), (n, q, got, want)


# ---- 2. the tails on the eps buffer against the restatement -----------------------------------------------------------
TAILS = [("ancestral", None, None), ("ddim", "ddim", 0.5), ("dpmpp2m", "dpmpp2m", 0.0)]
SHAPES = [(3, VC, 16, 16), (3, VC, 4, 5), (1, [2], 128, 192)]       # the last one: more float4 than one grid pass
# (guidance | None, threshold, threshold_max, guidance_rescale)
SETTINGS = ([(g, q, None, None) for g in (None, 3.0) for q in (0.5, 0.995, 1.0)] +
            [(g, None, None, phi) for g in (3.0, [0.5, 1.0, 7.5]) for phi in (0.7, 1.0)] +
            [(3.0, 0.995, None, 0.7), (3.0, 0.995, 1.5, None)])


def _steps_of(vf, dev, kind, solver, eta):
    """-> [(step index, plan | None, tau | None)]: three t of the ancestral tail / every k of a K = 5 plan."""
    from view_fusion_amd import schedule
    if kind == "ancestral":
        return [(t, None, None) for t in (T - 1, 4, 0)]
    tau = schedule.sample_timesteps(T, 5)
    plan = vf._sampler_plan(tau.tolist(), solver, eta, dev)
    return [(k, plan, tau) for k in range(5)]


def _ref_step(vf, betas, kind, solver, eta, idx, tau, y, eps, prev, z, q, c):
    """-> (y_next, mean | None, y0 | None, s | None) in float64."""
    if kind == "ancestral":
        sched = {k: v.cpu() for k, v in vf._sched().items()}
        y_next, mean, _, s = threshold_ref.ancestral_step(sched, idx, y, eps, z, q, c)
        return y_next, mean, None, s
    y_next, y0, s = threshold_ref.sampler_step(betas, tau, solver, eta, idx, y, eps, prev, z, q, c)
    return y_next, None, y0, s


def _run_tail(vf, out, off, y, z, idx, plan, B, max_v, weighting, hist=None, **kw):
    """One call of either tail -> (y_next, weights, y0_prev after the call | None, mean | None)."""
    from view_fusion_amd import ops
    tidx = idx if torch.is_tensor(idx) else torch.full((B,), idx, device=y.device)
    if plan is None:
        r, m, w = ops.p_sample_tail(out, off, y, z, tidx, vf._sched(), B, max_v, weighting, want_mean=True, **kw)
        return r, w, None, m
    h = None if hist is None else hist.clone()
    r, w = ops.sampler_step(out, off, y, z, tidx, plan, B, max_v, weighting, y0_prev=h, **kw)
    return r, w, h, None


def _dyn(dev, B, S, g, q, c, phi):
    """The keyword arguments of one setting for a tail call."""
    from view_fusion_amd import ops
    kw = dict(threshold=q, threshold_max=c, guidance_rescale=phi)
    if g is not None:
        kw.update(guidance=ops.guidance_scales(dev, B, g), S=S)
    return kw


@pytest.mark.parametrize("kind,solver,eta", TAILS, ids=[t[0] for t in TAILS])
@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("B,vc,H,W", SHAPES, ids=["16x16", "4x5", "128x192"])
def test_tails_against_the_restatement(vf, dev, B, vc, H, W, weighting, kind, solver, eta):
    from oracle import view_fusion_ref as vfr
    from view_fusion_amd import ops
    S = sum(vc)
    betas = vfr.beta_schedule(**SCHED_C1)
    gen = torch.Generator().manual_seed(23 + H)
    out = torch.randn(S + B, 6, H, W, generator=gen) * 2
    y, z, prev = (torch.randn(B, 3, H, W, generator=gen) for _ in range(3))
    off, _, max_v = ops.view_offsets(vc, dev)
    out_d, y_d, z_d, prev_d = out.to(dev), y.to(dev), z.to(dev), prev.to(dev)
    out_c = out_d[:S].contiguous()
    y64, z64, prev64 = y.double().numpy(), z.double().numpy(), prev.double().numpy()
    steps = _steps_of(vf, dev, kind, solver, eta)
    worst = 0.0
    for g, q, c, phi in SETTINGS:
        if g is not None and not np.isscalar(g):
            g = g[:B] if B > 1 else [7.5]
        rows, rows_d = (out, out_d) if g is not None else (out[:S], out_c)
        eps, w_ref, r_ref = threshold_ref.composed_eps(rows.double(), vc, weighting, g, phi)
        kw = _dyn(dev, B, S, g, q, c, phi)
        for idx, plan, tau in steps:
            _, w_plain, _, _ = _run_tail(vf, out_c, off, y_d, z_d, idx, plan, B, max_v, weighting, prev_d)
            got, w, h, m = _run_tail(vf, rows_d, off, y_d, z_d, idx, plan, B, max_v, weighting, prev_d, **kw)
            want, want_m, want_y0, s = _ref_step(vf, betas, kind, solver, eta, idx, tau, y64, eps, prev64, z64, q, c)
            errs = [rel(got, want)] + ([] if m is None else [rel(m, want_m)]) + ([] if h is None else [rel(h, want_y0)])
            worst = max(worst, *errs)
            assert torch.isfinite(got).all() and max(errs) <= KERNEL_RTOL, (kind, idx, g, q, c, phi, errs, s, r_ref)
            if c is not None:
                assert (s <= c).all()
            # the weights are the conditional ones, to the bit, whatever the setting
            if weighting:
                assert torch.equal(w, w_plain) and rel(w, w_ref) <= KERNEL_RTOL
            else:
                assert w is None and w_plain is None
            # in place = out of place, bit for bit
            y_in = y_d.clone()
            r_in, _, h_in, _ = _run_tail(vf, rows_d, off, y_in, z_d, idx, plan, B, max_v, weighting, prev_d, inplace=True,
                                         want_weights=False, scratch=ops.threshold_scratch(y_in), **kw)
            assert r_in is y_in and torch.equal(y_in, got) and (h is None or torch.equal(h_in, h))
    print(f"{kind} {H}x{W} weighting {weighting}: worst rel against the float64 restatement {worst:.2e}")
    with pytest.raises(ValueError):                          # a scratch made for another batch is refused
        _run_tail(vf, out_c, off, y_d, z_d, idx, plan, B, max_v, weighting, prev_d, threshold=0.9,
                  scratch=ops.threshold_scratch(torch.empty(B + 1, 3, H, W, device=dev)))


# ---- 3. identities, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,solver,eta", TAILS, ids=[t[0] for t in TAILS])
@pytest.mark.parametrize("H,W", [(16, 16), (4, 5)])
def test_a_threshold_of_one_is_the_static_clamp(vf, dev, kind, solver, eta, H, W):
    from oracle import view_fusion_ref as vfr
    from view_fusion_amd import ops
    B, S, q = 3, sum(VC), 0.9
    betas = vfr.beta_schedule(**SCHED_C1)
    gen = torch.Generator().manual_seed(5 + H)
    out = 0.1 * torch.randn(S + B, 6, H, W, generator=gen)
    y, z, prev = (0.1 * torch.randn(B, 3, H, W, generator=gen) for _ in range(3))
    off, _, max_v = ops.view_offsets(VC, dev)
    out_d, y_d, z_d, prev_d = out.to(dev), y.to(dev), z.to(dev), prev.to(dev)
    for g in (None, 3.0):
        rows, rows_d = (out, out_d) if g is not None else (out[:S], out_d[:S].contiguous())
        eps, _, _ = threshold_ref.composed_eps(rows.double(), VC, True, g)
        for idx, plan, tau in _steps_of(vf, dev, kind, solver, eta):
            *_, s = _ref_step(vf, betas, kind, solver, eta, idx, tau, y.double().numpy(), eps, prev.double().numpy(),
                              z.double().numpy(), q, None)
            assert (s == 1.0).all(), (kind, idx, g, s)       # the premise: no sample's quantile reaches 1
            kw = _dyn(dev, B, S, g, None, None, None)
            a = _run_tail(vf, rows_d, off, y_d, z_d, idx, plan, B, max_v, True, prev_d, **kw)
            b = _run_tail(vf, rows_d, off, y_d, z_d, idx, plan, B, max_v, True, prev_d, **dict(kw, threshold=q))
            for u, v in zip(a, b):
                assert (u is None and v is None) or torch.equal(u, v), (kind, idx, g)


@pytest.mark.parametrize("kind,solver,eta", TAILS, ids=[t[0] for t in TAILS])
def test_rescale_at_guidance_one_changes_nothing(vf, dev, kind, solver, eta):
    """eps_g = eps_c at g = 1, so r = phi + (1 - phi), which may round: KERNEL_RTOL, not bitwise."""
    from view_fusion_amd import ops
    B, S = 3, sum(VC)
    gen = torch.Generator().manual_seed(9)
    out = (torch.randn(S + B, 6, HW, HW, generator=gen) * 2).to(dev)
    y, z, prev = (torch.randn(B, 3, HW, HW, generator=gen).to(dev) for _ in range(3))
    off, _, max_v = ops.view_offsets(VC, dev)
    for idx, plan, _ in _steps_of(vf, dev, kind, solver, eta):
        for phi in (0.7, 1.0):
            a = _run_tail(vf, out, off, y, z, idx, plan, B, max_v, True, prev, **_dyn(dev, B, S, 1.0, None, None, None))
            b = _run_tail(vf, out, off, y, z, idx, plan, B, max_v, True, prev, **_dyn(dev, B, S, 1.0, None, None, phi))
            for u, v in zip(a, b):
                assert (u is None and v is None) or rel(v, u) <= KERNEL_RTOL, (kind, idx, phi)


@pytest.mark.parametrize("kind", ["ancestral", "ddim"])
@pytest.mark.parametrize("weighting,H,W", [(True, HW, HW), (False, 4, 5)], ids=["softmax-16x16", "mean-4x5"])
def test_the_eps_tails_draw_their_own_z(vf, dev, kind, weighting, H, W):
    """The _eps_rng entry points = the _eps ones fed with the generator's normals, keyed as their siblings."""
    from view_fusion_amd import ops, schedule
    B, seed, ids = 3, 0xC0FFEE, [4, 2 ** 33 + 1, 9]
    g = torch.Generator().manual_seed(3)
    out, y = torch.randn(sum(VC) + B, 6, H, W, generator=g).to(dev), torch.randn(B, 3, H, W, generator=g).to(dev)
    off, S, max_v = ops.view_offsets(VC, dev)
    idt = torch.tensor(ids, dtype=torch.int64, device=dev)
    kw = _dyn(dev, B, S, [0.5, 1.0, 7.5], 0.995, None, 0.7)
    if kind == "ancestral":
        ts = [7, 3, 0]                                      # t = 0: that sample gets no noise
        steps, tidx, plan = ts, torch.tensor(ts, device=dev), None
    else:
        tau = schedule.sample_timesteps(T, 5).tolist()
        plan = vf._sampler_plan(tau, "ddim", 0.5, dev)
        ks = [4, 2, 0]                                      # sigma[0] == 0
        steps, tidx = [tau[k] for k in ks], torch.tensor(ks, device=dev)
    run = lambda z=None, **more: _run_tail(vf, out, off, y, z, tidx, plan, B, max_v, weighting, **kw, **more)[0]
    got = run(seed=seed, ids=idt)
    z = torch.stack([ops.randn_ids(seed, idt[b:b + 1], ops.diffusion.RNG_STEP_NOISE, s, (3, H, W))[0]
                     for b, s in enumerate(steps)])
    z[2] = 0                                                # the drawn z is 0 at t = 0 (and unused where sigma[k] == 0)
    quiet = run()
    assert torch.equal(got, run(z=z)) and torch.equal(got[2], quiet[2]) and not torch.equal(got[0], quiet[0])


# ---- 4. generate() against the restatement through the oracle UNet ----------------------------------------------------
CHAINS = [dict(), dict(sample_steps=3, solver="ddim", eta=0.5), dict(sample_steps=3, solver="dpmpp2m")]
G = 3.0


def _ref_chain(case, kw, noisy, **dyn):
    tau = sampler_ref.timesteps(T, kw["sample_steps"]) if kw else None
    with torch.no_grad():
        return threshold_ref.chain(case["unet"], case["betas"], case["y_cond"], VC, case["angle"], case["y_T"],
                                   case["z_seq"] if noisy else None, G, tau=tau, solver=kw.get("solver", "ddim"),
                                   eta=kw.get("eta", 0.0), **dyn)


def _chain_error(ret, states):
    n = len(states)
    every = max(1, n // 8)
    keep = [i for i, k in enumerate(reversed(range(n))) if k % every == 0]
    assert ret.shape[1] == 1 + len(keep)
    return float((ret[:, 1:].cpu() - states[keep].transpose(0, 1)).abs().max())


@pytest.mark.parametrize("kw", CHAINS, ids=["ancestral", "ddim", "dpmpp2m"])
def test_generate_with_a_threshold_against_the_oracle(vf, case, kw):
    """Order statistics are 1-Lipschitz in the sup norm and s >= 1, so an error delta in y0_hat is at most 2 delta in y0:
    twice the guided chain's tolerance."""
    g = case["gpu"]
    noisy = not kw or kw.get("eta", 0.0) != 0
    inj = dict(y_t=g["y_T"], z_seq=g["z_seq"] if noisy else None, guidance=G, **kw)
    y, ret, logits, weights, samples = _gen(vf, case, threshold=0.9, **inj)
    states, _ = _ref_chain(case, kw, noisy, q=0.9)
    err = _chain_error(ret, states)
    print(f"generate(guidance={G}, threshold=0.9, {kw}): chain max-abs {err:.3e}  bound {2 * chain_tol(G):.1e}")
    assert torch.equal(ret[:, 0], g["y_T"]) and torch.equal(samples, ret[:, -1]) and torch.equal(y, samples)
    assert logits.shape[0] == sum(VC) and weights.shape[:3] == (3, ret.shape[1] - 1, 3)
    assert err <= 2 * chain_tol(G)
    static = _gen(vf, case, **inj)[4]                        # and the feature does something
    assert float((static - samples).abs().max()) > 10 * CHAIN_TOL


@pytest.mark.parametrize("kw", CHAINS, ids=["ancestral", "ddim", "dpmpp2m"])
def test_generate_with_a_rescale_against_the_oracle(vf, case, kw):
    """How much fp32 error moves r is not derivable: the bound is the larger of the guided chain's tolerance and 4 x the
    distance of the restatement run in float32 from the one in float64 on these inputs (profiles/threshold.md)."""
    g = case["gpu"]
    noisy = not kw or kw.get("eta", 0.0) != 0
    inj = dict(y_t=g["y_T"], z_seq=g["z_seq"] if noisy else None, guidance=G, **kw)
    samples = _gen(vf, case, guidance_rescale=0.7, **inj)
    states, _ = _ref_chain(case, kw, noisy, phi=0.7)
    states32, _ = _ref_chain(case, kw, noisy, phi=0.7, dtype=np.float32)
    dist = float((states32 - states).abs().max())
    bound = max(chain_tol(G), 4 * dist)
    err = _chain_error(samples[1], states)
    print(f"generate(guidance={G}, guidance_rescale=0.7, {kw}): chain max-abs {err:.3e}  float32 restatement against "
          f"float64 {dist:.3e}  bound {bound:.1e}")
    assert err <= bound
    plain = _gen(vf, case, **inj)[4]
    assert float((plain - samples[4]).abs().max()) > 10 * CHAIN_TOL


# ---- 5. plumbing ------------------------------------------------------------------------------------------------------
BOTH = dict(threshold=0.9, threshold_max=2.0, guidance_rescale=0.7)


@pytest.mark.parametrize("kw", [dict(seed=8, sample_ids=[100, 200, 300]), dict(sample_steps=5, solver="ddim", eta=0.5, seed=8)],
                         ids=["ancestral-seeded", "ddim-seeded"])
def test_graph_replay_equals_eager_bitwise(vf, case, kw):
    gs = torch.tensor([0.5, 1.0, 3.0])
    a = _gen(vf, case, use_graph=True, guidance=gs, **BOTH, **kw)
    b = _gen(vf, case, use_graph=False, guidance=gs, **BOTH, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.isfinite(a[1]).all()
    c = _gen(vf, case, use_graph=True, guidance=gs, **kw)
    assert not torch.equal(a[4], c[4])


@pytest.mark.parametrize("kind", ["ancestral", "ddim"])
def test_a_seeded_sample_does_not_depend_on_its_batch(vf, case, dev, kind):
    """Every statistic is per sample: the tail of a ragged batch of three equals, bit for bit, each sample's own."""
    from view_fusion_amd import ops, schedule
    B, S, seed = 3, sum(VC), 31337
    gen = torch.Generator().manual_seed(17)
    out = (torch.randn(S + B, 6, HW, HW, generator=gen) * 2).to(dev)
    y, prev = (torch.randn(B, 3, HW, HW, generator=gen).to(dev) for _ in range(2))
    off, _, max_v = ops.view_offsets(VC, dev)
    ids = torch.tensor([5, 9, 2 ** 40], dtype=torch.int64, device=dev)
    gs = [3.0, 1.5, 7.5]
    plan = None if kind == "ancestral" else vf._sampler_plan(schedule.sample_timesteps(T, 5).tolist(), "ddim", 1.0, dev)
    idx = 6 if plan is None else 3
    both = _run_tail(vf, out, off, y, None, idx, plan, B, max_v, True, prev, ids=ids, seed=seed,
                     **_dyn(dev, B, S, gs, 0.9, None, 0.7))
    lo = 0
    for b, v in enumerate(VC):
        rows = torch.cat([out[lo:lo + v], out[S + b:S + b + 1]]).contiguous()
        off1, _, _ = ops.view_offsets([v], dev)
        one = _run_tail(vf, rows, off1, y[b:b + 1].contiguous(), None, idx, plan, 1, v, True, prev[b:b + 1].contiguous(),
                        ids=ids[b:b + 1].contiguous(), seed=seed, **_dyn(dev, 1, v, gs[b], 0.9, None, 0.7))
        assert torch.equal(both[0][b], one[0][0]) and torch.equal(both[1][b, :v], one[1][0])
        assert both[2] is None or torch.equal(both[2][b], one[2][0])
        lo += v
    # and through generate(), as the guidance test compares: y_T bitwise, the chain within its tolerance
    g = case["gpu"]
    kw = dict(seed=seed, **BOTH, **({} if kind == "ancestral" else dict(sample_steps=3, solver="ddim", eta=1.0)))
    _, whole, *_ = vf.generate(g["y_cond"], case["vc"], g["angle"], sample_ids=ids, guidance=torch.tensor(gs), **kw)
    for b in range(B):
        _, one, *_ = vf.generate(g["y_cond"][b:b + 1], case["vc"][b:b + 1], g["angle"][b:b + 1], sample_ids=ids[b:b + 1],
                                 guidance=gs[b], **kw)
        assert torch.equal(whole[b, 0], one[0, 0])
        err = float((whole[b] - one[0]).abs().max())
        print(f"{kind} id {int(ids[b])}, g {gs[b]}, alone vs in the ragged batch: max-abs {err:.3e}  bound {2 * chain_tol(gs[b]):.1e}")
        assert err <= 2 * chain_tol(gs[b])


def test_p_sample_and_p_mean_variance_take_the_arguments(vf, case, dev):
    g = case["gpu"]
    t = torch.full((3,), 5, device=dev)
    args = (g["y_T"], g["y_cond"], case["vc"], g["angle"], t)
    y0, logits0, w0 = vf.p_sample(*args, z=g["z_seq"][5], guidance=G)
    for dyn in (dict(threshold=0.9), dict(guidance_rescale=0.7), BOTH):
        y1, logits, w = vf.p_sample(*args, z=g["z_seq"][5], guidance=G, **dyn)
        assert logits.shape == logits0.shape == (sum(VC), 3, HW, HW) and w.shape == w0.shape
        assert float((y1 - y0).abs().max()) > 10 * CHAIN_TOL and torch.isfinite(y1).all()
        mean, logvar, logits2, _ = vf.p_mean_variance(*args, True, guidance=G, **dyn)
        sd = (0.5 * logvar).exp()
        assert logits2.shape == logits.shape and float((mean + g["z_seq"][5] * sd - y1).abs().max()) <= 1e-5
    u0 = vf.p_sample(*args, z=g["z_seq"][5])[0]                # the threshold alone needs no guidance
    u1 = vf.p_sample(*args, z=g["z_seq"][5], threshold=1.0)[0]     # s = max|y0_hat| > 1 here: nothing is clamped
    assert float((u1 - u0).abs().max()) > 10 * CHAIN_TOL


def test_drivers_take_the_arguments(vf, dev):
    from view_fusion_amd import drivers
    g = torch.Generator().manual_seed(701)
    full = dict(target=torch.rand(3, 3, HW, HW, generator=g).to(dev), cond=torch.rand(3, 6, 3, HW, HW, generator=g).to(dev),
                angle=torch.rand(3, 1, generator=g).to(dev), view_count=torch.tensor([2, 6, 1]), ids=torch.tensor([11, 5, 8]))
    a = drivers.evaluate(vf, [full], seed=21, sample_steps=3, guidance=G, **BOTH)
    b = drivers.evaluate(vf, [full], seed=21, sample_steps=3, guidance=G)
    assert torch.isfinite(a["psnr"]) and torch.isfinite(b["psnr"]) and float(a["psnr"]) != float(b["psnr"])
    first = torch.rand(2, 3, HW, HW, generator=g).to(dev)
    kw = dict(steps=2, sample_steps=2, seed=4, guidance=G)
    r = drivers.autoregressive_rollout(vf, first, **kw, **BOTH)
    assert r.shape == (2, 2, 3, HW, HW) and torch.isfinite(r).all()
    assert not torch.equal(r, drivers.autoregressive_rollout(vf, first, **kw))
    cond23 = torch.rand(2, 23, 3, HW, HW, generator=g).to(dev)
    ang = torch.rand(2, 1, generator=g).to(dev)
    kw = dict(view_count=torch.tensor([7, 9]), sample_steps=2, seed=4, guidance=G)
    ex = drivers.extrapolate(vf, cond23, ang, **kw, **BOTH)[0]
    assert torch.isfinite(ex).all() and not torch.equal(ex, drivers.extrapolate(vf, cond23, ang, **kw)[0])
    views = torch.rand(24, 3, HW, HW, generator=g).to(dev)
    kw = dict(sample_steps=2, seed=4, guidance=G)
    fr = drivers.orbit_frames(vf, views, **kw, **BOTH)[0]
    assert fr.shape[0] == 24 and torch.isfinite(fr).all() and not torch.equal(fr, drivers.orbit_frames(vf, views, **kw)[0])


# ---- 6. what each path launches ---------------------------------------------------------------------------------------
def test_launches_of_each_path(vf, case, dev):
    g = case["gpu"]
    run = lambda **kw: _names(lambda: _gen(vf, case, use_graph=False, **kw))
    paths = [(dict(y_t=g["y_T"], z_seq=g["z_seq"]), "vf_p_sample_tail_eps", T),
             (dict(seed=5), "vf_p_sample_tail_eps_rng", T),
             (dict(sample_steps=3, solver="dpmpp2m", y_t=g["y_T"]), "vf_sampler_step_eps", 3),
             (dict(sample_steps=3, eta=0.5, seed=5), "vf_sampler_step_eps_rng", 3)]
    for kw, tail, n in paths:
        for guidance in (None, G):
            base = run(guidance=guidance, **kw)
            assert not NEW & set(base)                       # the default and the guidance-only path: no new name
            for dyn in (dict(threshold=0.9), BOTH if guidance else dict(threshold=0.9, threshold_max=2.0)):
                on = run(guidance=guidance, **kw, **dyn)
                assert on.count("vf_compose_eps") == on.count("vf_sample_stat") == on.count(tail) == n, (kw, guidance, dyn)
                assert not OLD_TAILS & set(on) and (NEW & set(on)) == {"vf_compose_eps", "vf_sample_stat", tail}
                assert len(on) == len(base) + 2 * n          # two launches more per step, nothing else
            # guidance_rescale=0 is "off": the launches of before
            if guidance:
                assert run(guidance=guidance, guidance_rescale=0, **kw) == base
