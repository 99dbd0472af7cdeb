"""Classifier-free guidance on the GPU (csrc/diffusion.hip holds the definition, tests/guidance_ref.py restates it):
stacking with dropped samples and null rows, the four guided tails against the float64 restatement and against their
unguided siblings, generate(guidance=) against the restatement through the oracle UNet, graph replay, the launches each
path logs, conditioning dropout in forward() and in the Trainer, the drivers.

TINY 16 x 16, SCHED_C1 (T = 10), B = 3 with ragged view counts (1, 3, 2).
Tolerances: one kernel rel 2e-5 (max|a-b| / max|b|); chains max-abs (g + |1 - g|) 1e-3 -- the project's chain
tolerance times the factor by which the guided combination amplifies an error in either prediction; "bitwise" is
torch.equal."""
import numpy as np
import pytest
import torch

import guidance_ref
import sampler_ref
from conftest import SCHED_C1, TINY

pytestmark = pytest.mark.gpu
KERNEL_RTOL, CHAIN_TOL = 2e-5, 1e-3
HW = TINY["image_size"]
T = SCHED_C1["num_timesteps"]
VC = [1, 3, 2]
SEED = 3                                   # ids 0..5, p = 0.5: the mixed mask 0 1 1 0 1 0 (test_guidance_host.py)
NEW = {"vf_stack_views_cfg", "vf_draw_cond_drop", "vf_p_sample_tail_cfg", "vf_p_sample_tail_cfg_rng", "vf_sampler_step_cfg",
       "vf_sampler_step_cfg_rng"}


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


# ---- 1. stacking ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [3, 6])
@pytest.mark.parametrize("H,W", [(16, 16), (4, 5)])         # 4 x 5: 15 float4 per image, less than one workgroup
def test_stacking_with_drop_and_null_rows(dev, H, W, Cc):
    from view_fusion_amd import ops
    B, N = 3, 3
    g = torch.Generator().manual_seed(5 + H + Cc)
    y_cond, y_t = torch.rand(B, N, Cc, H, W, generator=g).to(dev), torch.rand(B, 3, H, W, generator=g).to(dev)
    noise, level = torch.randn(B, 3, H, W, generator=g).to(dev), (0.05 + 0.9 * torch.rand(B, generator=g)).to(dev)
    angle = torch.rand(B, 1, generator=g).to(dev)
    off, S, _ = ops.view_offsets(VC, dev)
    off1, _, _ = ops.view_offsets([1] * B, dev)
    mask = torch.tensor([False, True, True], device=dev)
    zeroed = y_cond.clone()
    zeroed[mask] = 0
    for nz in (noise, None):
        want = ops.stack_views(zeroed, y_t, nz, level, angle, off, S)
        for m in (mask, mask.to(torch.uint8)):
            got = ops.stack_views(y_cond, y_t, nz, level, angle, off, S, drop=m)
            assert all(torch.equal(a, b) for a, b in zip(got, want))
        none = ops.stack_views(y_cond, y_t, nz, level, angle, off, S, drop=torch.zeros(B, dtype=torch.bool, device=dev))
        plain = ops.stack_views(y_cond, y_t, nz, level, angle, off, S)
        assert all(torch.equal(a, b) for a, b in zip(none, plain))
        # null rows: the existing call on a one-view batch of zero conditioning
        null = ops.stack_views(torch.zeros(B, 1, Cc, H, W, device=dev), y_t, nz, level, angle, off1, B)
        for m, head in ((None, plain), (mask, want)):
            x, ls, as_ = ops.stack_views(y_cond, y_t, nz, level, angle, off, S, drop=m, null_rows=True)
            assert x.shape == (S + B, Cc + 3, H, W) and ls.shape == as_.shape == (S + B, 1)
            for got_t, head_t, null_t in zip((x, ls, as_), head, null):
                assert torch.equal(got_t[:S], head_t) and torch.equal(got_t[S:], null_t)
    # copy_cond=False leaves the conditioning half of all S + B rows alone
    x = torch.full((S + B, Cc + 3, H, W), float("nan"), device=dev)
    ops.stack_views(y_cond, y_t, None, level, angle, off, S, x=x, copy_cond=False, null_rows=True, drop=mask)
    assert torch.isnan(x[:, :Cc]).all() and torch.equal(x[:S, Cc:], plain[0][:S, Cc:]) and torch.equal(x[S:, Cc:], y_t)
    with pytest.raises(ValueError):
        ops.stack_views(y_cond, y_t, None, level, angle, off, S, drop=torch.zeros(B + 1, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError):
        ops.stack_views(y_cond, y_t, None, level, angle, off, S, x=plain[0], null_rows=True)


# ---- 2. the guided tails ------------------------------------------------------------------------------------------------
TAILS = [("ancestral", None, None), ("ddim", "ddim", 0.5), ("dpmpp2m", "dpmpp2m", 0.0)]
SHAPES = [(3, VC, 16, 16), (3, VC, 4, 5), (1, [2], 128, 192)]       # the last one: more float4 than one grid pass


def _tail_cases(vf, dev, kind, solver, eta):
    """-> [(step index, plan | None, reference step fn)]: three t of the ancestral tail / every k of a K = 5 plan."""
    from oracle import view_fusion_ref as vfr
    from view_fusion_amd import schedule
    betas = vfr.beta_schedule(**SCHED_C1)
    if kind == "ancestral":
        sched = {k: v.cpu() for k, v in vf._sched().items()}
        return [(t, None, lambda y, eps, hist, z, t=t: (guidance_ref.ancestral_step(sched, t, y, eps, z)[0], None))
                for t in (T - 1, 4, 0)]
    tau = schedule.sample_timesteps(T, 5)
    plan = vf._sampler_plan(tau.tolist(), solver, eta, dev)
    return [(k, plan, lambda y, eps, hist, z, k=k: sampler_ref.step(betas, tau, solver, eta, k, y, eps, hist, z))
            for k in range(5)]


def _run_tail(vf, out, off, y, z, idx, plan, B, max_v, weighting, hist=None, **kw):
    """One call of either tail -> (y_next, weights, y0_prev after the call | None)."""
    from view_fusion_amd import ops
    tidx = torch.full((B,), idx, device=y.device)
    if plan is None:
        r, _, w = ops.p_sample_tail(out, off, y, z, tidx, vf._sched(), B, max_v, weighting, **kw)
        return r, w, None
    h = None if hist is None else hist.clone()
    r, w = ops.sampler_step(out, off, y, z, tidx, plan, B, max_v, weighting, y0_prev=h, **kw)
    return r, w, h


@pytest.mark.parametrize("kind,solver,eta", TAILS, ids=[t[0] for t in TAILS])
@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("B,vc,H,W", SHAPES, ids=["16x16", "4x5", "128x192"])
def test_guided_tails_against_the_restatement(vf, dev, B, vc, H, W, weighting, kind, solver, eta):
    from view_fusion_amd import ops
    S = sum(vc)
    g = torch.Generator().manual_seed(23 + H)
    out = torch.randn(S + B, 6, H, W, generator=g) * 2
    y, z, prev = (torch.randn(B, 3, H, W, generator=g) for _ in range(3))
    off, _, max_v = ops.view_offsets(vc, dev)
    off1, _, _ = ops.view_offsets([1] * B, dev)
    out_d, y_d, z_d, prev_d = out.to(dev), y.to(dev), z.to(dev), prev.to(dev)
    scales = [0.0, 1.0, 3.0, [0.5, 1.0, 7.5][:B] if B > 1 else [7.5]]
    worst = 0.0
    for idx, plan, ref_step in _tail_cases(vf, dev, kind, solver, eta):
        plain, w_plain, h_plain = _run_tail(vf, out_d[:S].contiguous(), off, y_d, z_d, idx, plan, B, max_v, weighting, prev_d)
        null, _, _ = _run_tail(vf, out_d[S:].contiguous(), off1, y_d, z_d, idx, plan, B, 1, weighting, prev_d)
        for gv in scales:
            gs = ops.guidance_scales(dev, B, gv)
            got, w, h = _run_tail(vf, out_d, off, y_d, z_d, idx, plan, B, max_v, weighting, prev_d, guidance=gs, S=S)
            eps, w_ref = guidance_ref.guided_eps(out.double(), vc, weighting, gv)
            want, want_y0 = ref_step(y.double().numpy(), eps.numpy(), prev.double().numpy(), z.double().numpy())
            e = rel(got, want)
            e0 = 0.0 if h is None else rel(h, want_y0)
            worst = max(worst, e, e0)
            assert torch.isfinite(got).all() and e <= KERNEL_RTOL and e0 <= KERNEL_RTOL, (kind, idx, gv, e, e0)
            # the weights are the conditional ones, whatever the scale
            if weighting:
                assert torch.equal(w, w_plain) and rel(w, w_ref) <= KERNEL_RTOL
            else:
                assert w is None and w_plain is None
            if gv == 1.0:                                # today's sampler, to the bit
                assert torch.equal(got, plain) and (h is None or torch.equal(h, h_plain))
                if plan is None:
                    m_g = ops.p_sample_tail(out_d, off, y_d, z_d, torch.full((B,), idx, device=dev), vf._sched(), B, max_v,
                                            weighting, want_mean=True, guidance=gs, S=S)[1]
                    m_p = ops.p_sample_tail(out_d[:S].contiguous(), off, y_d, z_d, torch.full((B,), idx, device=dev),
                                            vf._sched(), B, max_v, weighting, want_mean=True)[1]
                    assert torch.equal(m_g, m_p)
            if gv == 0.0:                                # the unconditional model, to the bit
                assert torch.equal(got, null)
            # in place = out of place, bit for bit
            y_in = y_d.clone()
            r_in, _, h_in = _run_tail(vf, out_d, off, y_in, z_d, idx, plan, B, max_v, weighting, prev_d, guidance=gs,
                                      S=S, inplace=True, want_weights=False)
            assert r_in is y_in and torch.equal(y_in, got) and (h is None or torch.equal(h_in, h))
    print(f"{kind} {H}x{W} weighting {weighting}: worst rel against the float64 restatement {worst:.2e}")
    with pytest.raises(ValueError):
        _run_tail(vf, out_d, off, y_d, z_d, idx, plan, B, max_v, weighting, guidance=torch.ones(B + 1, device=dev), S=S)
    # the kernel reads rows S .. S + B - 1 and cannot see the row count: anything but S + B rows is refused on the host
    for rows in (out_d[:S], out_d[:S + B - 1], torch.cat([out_d, out_d[:1]])):
        with pytest.raises(ValueError):
            _run_tail(vf, rows.contiguous(), off, y_d, z_d, idx, plan, B, max_v, weighting, guidance=gs, S=S)
    with pytest.raises(ValueError):
        _run_tail(vf, out_d, off, y_d, z_d, idx, plan, B, max_v, weighting, guidance=gs)          # no S


@pytest.mark.parametrize("kind", ["ancestral", "ddim"])
@pytest.mark.parametrize("weighting,H,W", [(True, HW, HW), (False, HW, HW), (True, 4, 5), (False, 4, 5)],
                         ids=["softmax-16x16", "mean-16x16", "softmax-4x5", "mean-4x5"])
def test_guided_tails_draw_their_own_z(vf, dev, kind, weighting, H, W):
    """The _cfg_rng entry points = the _cfg ones fed with the generator's normals, keyed as their unguided siblings."""
    from view_fusion_amd import ops, schedule
    B, seed, ids = 3, 0xC0FFEE, [4, 2 ** 33 + 1, 9]
    g = torch.Generator().manual_seed(3)
    out, y = torch.randn(sum(VC) + B, 6, H, W, generator=g).to(dev), torch.randn(B, 3, H, W, generator=g).to(dev)
    off, S, max_v = ops.view_offsets(VC, dev)
    idt = torch.tensor(ids, dtype=torch.int64, device=dev)
    gs = ops.guidance_scales(dev, B, [0.5, 1.0, 7.5])
    if kind == "ancestral":
        ts = [7, 3, 0]                                      # t = 0: that sample gets no noise
        steps, tidx = ts, torch.tensor(ts, device=dev)
        run = lambda **kw: ops.p_sample_tail(out, off, y, kw.pop("z", None), tidx, vf._sched(), B, max_v, weighting, guidance=gs, S=S, **kw)[0]
        plain = ops.p_sample_tail(out[:S].contiguous(), off, y, None, tidx, vf._sched(), B, max_v, weighting, seed=seed, ids=idt)[0]
    else:
        tau = schedule.sample_timesteps(T, 5).tolist()
        plan = vf._sampler_plan(tau, "ddim", 0.5, dev)
        ks = [4, 2, 0]                                      # sigma[0] == 0
        steps, tidx = [tau[k] for k in ks], torch.tensor(ks, device=dev)
        run = lambda **kw: ops.sampler_step(out, off, y, kw.pop("z", None), tidx, plan, B, max_v, weighting, guidance=gs, S=S, **kw)[0]
        plain = ops.sampler_step(out[:S].contiguous(), off, y, None, tidx, plan, B, max_v, weighting, seed=seed, ids=idt)[0]
    got = run(seed=seed, ids=idt)
    z = torch.stack([ops.randn_ids(seed, idt[b:b + 1], ops.diffusion.RNG_STEP_NOISE, s, (3, H, W))[0]
                     for b, s in enumerate(steps)])
    z[2] = 0                                                # the drawn z is 0 at t = 0 (and unused where sigma[k] == 0)
    quiet = run()
    assert torch.equal(got, run(z=z)) and torch.equal(got[2], quiet[2]) and not torch.equal(got[0], quiet[0])
    assert torch.equal(got[1], plain[1]) and not torch.equal(got[0], plain[0])       # g = 1 is the sibling's sample


# ---- 3. generate(guidance=) against the restatement through the oracle UNet --------------------------------------------
CHAINS = [dict(), dict(sample_steps=3, solver="ddim", eta=0.5), dict(sample_steps=3, solver="dpmpp2m")]


@pytest.mark.parametrize("kw", CHAINS, ids=["ancestral", "ddim", "dpmpp2m"])
def test_generate_against_the_oracle(vf, case, kw):
    G = 3.0
    g = case["gpu"]
    noisy = not kw or kw.get("eta", 0.0) != 0
    y, ret, logits, weights, samples = _gen(vf, case, y_t=g["y_T"], z_seq=g["z_seq"] if noisy else None, guidance=G, **kw)
    tau = sampler_ref.timesteps(T, kw["sample_steps"]) if kw else None
    with torch.no_grad():
        states, w_ref = guidance_ref.chain(case["unet"], case["betas"], case["y_cond"], VC, case["angle"], case["y_T"],
                                           case["z_seq"] if noisy else None, G, tau=tau, solver=kw.get("solver", "ddim"),
                                           eta=kw.get("eta", 0.0))
    n = len(states)
    every = max(1, n // 8)
    keep = [i for i, k in enumerate(reversed(range(n))) if k % every == 0]
    assert ret.shape == (3, 1 + len(keep), 3, HW, HW) and weights.shape == (3, len(keep), 3, 3, HW, HW)
    assert logits.shape == (sum(VC), len(keep), 3, HW, HW)               # the S real rows' logits
    err = float((ret[:, 1:].cpu() - states[keep].transpose(0, 1)).abs().max())
    werr = float((weights.cpu() - torch.stack([w_ref[i] for i in keep], dim=1)).abs().max())
    print(f"generate(guidance={G}, {kw}): chain max-abs {err:.3e}  weights {werr:.3e}  bound {chain_tol(G):.1e}")
    assert torch.equal(ret[:, 0], g["y_T"]) and torch.equal(samples, ret[:, -1]) and torch.equal(y, samples)
    assert err <= chain_tol(G) and werr <= chain_tol(G)
    # and guidance does something: the unguided sample is another one
    plain = _gen(vf, case, y_t=g["y_T"], z_seq=g["z_seq"] if noisy else None, **kw)
    assert float((plain[4] - samples).abs().max()) > 10 * CHAIN_TOL


@pytest.mark.parametrize("kw", CHAINS, ids=["ancestral", "ddim", "dpmpp2m"])
def test_guidance_one_is_the_unguided_sampler(vf, case, kw):
    """Not bitwise: the kernel-choice policy sees S + B rows instead of S."""
    g = case["gpu"]
    a = _gen(vf, case, y_t=g["y_T"], z_seq=g["z_seq"], **kw)
    b = _gen(vf, case, y_t=g["y_T"], z_seq=g["z_seq"], guidance=1.0, **kw)
    assert [tuple(x.shape) for x in a] == [tuple(x.shape) for x in b]
    err, werr, lerr = (float((a[i] - b[i]).abs().max()) for i in (1, 3, 2))
    print(f"guidance=1.0 vs None, {kw}: chain max-abs {err:.3e}  weights {werr:.3e}  logits {lerr:.3e}")
    assert err <= chain_tol(1.0) and werr <= chain_tol(1.0)


@pytest.mark.parametrize("kw", [dict(seed=8, sample_ids=[100, 200, 300]), dict(sample_steps=5, solver="ddim", eta=0.5, seed=8),
                                dict(sample_steps=5, solver="dpmpp2m")], ids=["ancestral-seeded", "ddim-seeded", "dpmpp2m"])
def test_graph_replay_equals_eager_bitwise(vf, case, kw):
    if "seed" not in kw:
        kw = dict(kw, y_t=case["gpu"]["y_T"])
    a = _gen(vf, case, use_graph=True, guidance=torch.tensor([0.5, 1.0, 3.0]), **kw)
    b = _gen(vf, case, use_graph=False, guidance=torch.tensor([0.5, 1.0, 3.0]), **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.isfinite(a[1]).all()


def test_a_seeded_guided_sample_does_not_depend_on_the_batch(vf, case, dev):
    g = case["gpu"]
    kw = dict(seed=31337, sample_steps=3, solver="ddim", eta=1.0)
    rng_state = torch.cuda.get_rng_state(dev)
    _, both, *_ = vf.generate(g["y_cond"][1:], case["vc"][1:], g["angle"][1:], sample_ids=[5, 9],
                              guidance=torch.tensor([3.0, 1.5]), **kw)
    for row, sid, gv in ((0, 5, 3.0), (1, 9, 1.5)):
        _, one, *_ = vf.generate(g["y_cond"][1 + row:2 + row], case["vc"][1 + row:2 + row], g["angle"][1 + row:2 + row],
                                 sample_ids=torch.tensor([sid], device=dev), guidance=gv, **kw)
        assert torch.equal(both[row, 0], one[0, 0])                       # y_T bitwise
        err = float((both[row] - one[0]).abs().max())
        print(f"id {sid}, g {gv}, alone vs in a ragged batch of two: max-abs {err:.3e}  bound {chain_tol(gv):.1e}")
        assert err <= chain_tol(gv)
    assert torch.equal(torch.cuda.get_rng_state(dev), rng_state)          # torch's device generator was not touched
    _, other, *_ = vf.generate(g["y_cond"][2:3], case["vc"][2:3], g["angle"][2:3], sample_ids=[9], guidance=3.0, **kw)
    assert float((other - one).abs().max()) > 10 * CHAIN_TOL              # another scale: another sample


def test_p_sample_and_p_mean_variance_take_the_scale(vf, case, dev):
    from view_fusion_amd import ops
    g = case["gpu"]
    t = torch.full((3,), 5, device=dev)
    gs = torch.tensor([0.0, 1.0, 3.0])
    y1, logits, w = vf.p_sample(g["y_T"], g["y_cond"], case["vc"], g["angle"], t, z=g["z_seq"][5], guidance=gs)
    y0, logits0, w0 = vf.p_sample(g["y_T"], g["y_cond"], case["vc"], g["angle"], t, z=g["z_seq"][5])
    assert logits.shape == logits0.shape == (sum(VC), 3, HW, HW) and w.shape == w0.shape
    assert float((y1[1] - y0[1]).abs().max()) <= chain_tol(1.0) and float((y1[2] - y0[2]).abs().max()) > 10 * CHAIN_TOL
    mean, logvar, logits2, _ = vf.p_mean_variance(g["y_T"], g["y_cond"], case["vc"], g["angle"], t, True, guidance=gs)
    sd = (0.5 * logvar).exp()
    assert logits2.shape == logits.shape and float((mean + g["z_seq"][5] * sd - y1).abs().max()) <= 1e-5


# ---- 4. what each path launches ---------------------------------------------------------------------------------------
def test_launches_of_each_path(vf, case, dev):
    g = case["gpu"]
    run = lambda **kw: _names(lambda: _gen(vf, case, use_graph=False, **kw))
    guided = run(y_t=g["y_T"], z_seq=g["z_seq"], guidance=3.0)
    assert guided.count("vf_p_sample_tail_cfg") == T and guided.count("vf_stack_views_cfg") == T + 1
    assert not {"vf_p_sample_tail", "vf_p_sample_tail_rng", "vf_sampler_step", "vf_sampler_step_rng", "vf_stack_views"} & set(guided)
    seeded = run(seed=5, guidance=3.0)
    assert seeded.count("vf_p_sample_tail_cfg_rng") == T and "vf_p_sample_tail_cfg" not in seeded
    few = run(sample_steps=3, solver="dpmpp2m", y_t=g["y_T"], guidance=3.0)
    assert few.count("vf_sampler_step_cfg") == 3 and "vf_sampler_step" not in few and "vf_stack_views" not in few
    few_seeded = run(sample_steps=3, eta=0.5, seed=5, guidance=3.0)
    assert few_seeded.count("vf_sampler_step_cfg_rng") == 3 and "vf_sampler_step_rng" not in few_seeded
    # guidance=None: none of the new names
    for kw in (dict(y_t=g["y_T"], z_seq=g["z_seq"]), dict(seed=5), dict(sample_steps=3, eta=0.5, seed=5)):
        plain = run(**kw)
        assert not NEW & set(plain)
    # training with p = 0: the list of a model that never heard of dropout
    batch = _batch(dev)
    lists = []
    for touch in (False, True):
        m = _model(dev)
        if touch:
            m.set_cond_dropout(0.3)
            m.set_cond_dropout(0.0)
        lists.append(_names(lambda: m(**batch, seed=SEED).backward()))
        assert m.last_cond_drop is None
    assert lists[0] == lists[1] and not NEW & set(lists[0]) and "vf_stack_views" in lists[0]
    m = _model(dev)
    m.set_cond_dropout(0.5)
    on = _names(lambda: m(**batch, seed=SEED).backward())
    assert on.count("vf_draw_cond_drop") == 1 and on.count("vf_stack_views_cfg") == 1 and "vf_stack_views" not in on
    assert len(on) == len(lists[0]) + 1                              # one small launch more
    m.eval()                                                          # like Dropout: only in training mode
    assert not NEW & set(_names(lambda: m(**batch, seed=SEED))) and m.last_cond_drop is None


# ---- 5. conditioning dropout in forward() -----------------------------------------------------------------------------
def _batch(dev, B=3, vc=VC, s=0):
    from view_fusion_amd import train
    return dict(train.synthetic_batch(B, 3, HW, dev, seed=60 + s), view_count=torch.tensor(vc))


def _loss_and_grads(m, batch, **kw):
    for p in m.parameters():
        p.grad = None
    loss = m(**batch, **kw)
    loss.backward()
    return loss.detach().clone(), [p.grad.clone() for p in m.parameters()]


def _zeroed(batch, mask):
    out = dict(batch, y_cond=batch["y_cond"].clone())
    out["y_cond"][torch.as_tensor(np.asarray(mask), dtype=torch.bool)] = 0
    return out


@pytest.mark.parametrize("p", [0.5, 1.0])
def test_seeded_dropout_is_the_run_on_zeroed_conditioning(dev, p):
    m = _model(dev)
    batch = _batch(dev)
    ids = torch.tensor([1, 2, 3], dtype=torch.int64, device=dev)         # p = 0.5: mask 1 1 0
    want_mask = guidance_ref.cond_drop(SEED, [1, 2, 3], p)
    assert want_mask.tolist() == ([True, True, False] if p == 0.5 else [True] * 3)
    m.set_cond_dropout(p)
    loss, grads = _loss_and_grads(m, batch, seed=SEED, sample_ids=ids)
    assert m.last_cond_drop.is_cuda and m.last_cond_drop.dtype == torch.uint8
    assert np.array_equal(m.last_cond_drop.cpu().numpy().astype(bool), want_mask)
    m.set_cond_dropout(0.0)
    loss0, grads0 = _loss_and_grads(m, _zeroed(batch, want_mask), seed=SEED, sample_ids=ids)
    assert m.last_cond_drop is None
    assert torch.equal(loss, loss0) and all(torch.equal(a, b) for a, b in zip(grads, grads0))
    full, _ = _loss_and_grads(m, batch, seed=SEED, sample_ids=ids)
    assert not torch.equal(full, loss)                                   # (the conditioning does matter)
    # an injected mask wins over p and over the seed
    m.set_cond_dropout(p)
    inj = torch.tensor([False, False, True], device=dev)
    loss_i, grads_i = _loss_and_grads(m, batch, seed=SEED, sample_ids=ids, cond_drop=inj)
    assert torch.equal(m.last_cond_drop.bool(), inj)
    m.set_cond_dropout(0.0)
    loss_z, grads_z = _loss_and_grads(m, _zeroed(batch, inj.cpu().numpy()), seed=SEED, sample_ids=ids)
    assert torch.equal(loss_i, loss_z) and all(torch.equal(a, b) for a, b in zip(grads_i, grads_z))


def test_unseeded_dropout_draws_after_t_u_and_noise(dev):
    m = _model(dev)
    batch = _batch(dev, 4, [1, 3, 2, 2])
    B, p = 4, 0.5
    torch.manual_seed(1234)
    state = torch.cuda.get_rng_state(dev)
    m.set_cond_dropout(p)
    loss, grads = _loss_and_grads(m, batch)
    mask = m.last_cond_drop.bool().clone()
    # replay the draws from the saved state: t, u, noise as the default path draws them, then the mask
    torch.cuda.set_rng_state(state, dev)
    t = torch.randint(1, T, (B,), device=dev).long()
    u = torch.rand((B, 1), device=dev)
    noise = torch.randn_like(batch["y_0"])
    want = torch.rand(B, device=dev) < p
    assert torch.equal(mask, want)
    m.set_cond_dropout(0.0)
    loss0, grads0 = _loss_and_grads(m, _zeroed(batch, mask.cpu().numpy()), t=t, u=u, noise=noise)
    assert torch.equal(loss, loss0) and all(torch.equal(a, b) for a, b in zip(grads, grads0))
    # ... and p = 0 from the same state draws the very same t, u, noise (and nothing after them)
    torch.cuda.set_rng_state(state, dev)
    plain, _ = _loss_and_grads(m, batch)
    injected, _ = _loss_and_grads(m, batch, t=t, u=u, noise=noise)
    assert torch.equal(plain, injected)


# ---- 6. Trainer ---------------------------------------------------------------------------------------------------------
TB, TVC, TSEED = 4, [1, 3, 2, 2], 3


def _trainer(dev, graph, p=0.5, **kw):
    from view_fusion_amd import train
    m = _model(dev)
    m.set_cond_dropout(p)
    tr = train.Trainer(m, lr_warmup=1, graph=graph, seed=TSEED, **kw)
    tr.it = 0
    return m, tr


def _steps(dev, m, tr, n, first=0):
    losses, masks = [], []
    for s in range(first, first + n):
        losses.append(tr.step(_batch(dev, TB, TVC, s)).clone())
        masks.append(None if m.last_cond_drop is None else m.last_cond_drop.cpu().numpy().astype(bool))
    return losses, masks


def test_trainer_graph_replay_equals_eager(dev):
    from view_fusion_amd import train
    (m_e, tr_e), (m_g, tr_g) = _trainer(dev, False), _trainer(dev, True)
    (le, me), (lg, mg) = _steps(dev, m_e, tr_e, 3), _steps(dev, m_g, tr_g, 3)
    assert tr_e.graph_steps == 0 and tr_g.graph_steps == 1 and tr_g.mode == "graph"
    (le2, me2), (lg2, mg2) = _steps(dev, m_e, tr_e, 3, first=3), _steps(dev, m_g, tr_g, 3, first=3)
    assert tr_g.graph_steps == 4
    assert all(torch.equal(a, b) for a, b in zip(le + le2, lg + lg2))
    assert all(torch.equal(a, b) for a, b in zip(m_e.parameters(), m_g.parameters()))
    seen = set()
    for it, (a, b) in enumerate(zip(me + me2, mg + mg2), start=1):
        first = train.step_sample_ids(it, TB)
        want = guidance_ref.cond_drop(TSEED, np.arange(first, first + TB), 0.5)
        assert np.array_equal(a, want) and np.array_equal(b, want), (it, a, b, want)
        seen.add(tuple(want.tolist()))
    assert len(seen) > 1                                                 # the masks do change from step to step

    # set_cond_dropout(0) between steps: the captured steps are dropped, and from here on both are a Trainer that never
    # had dropout (given the same parameters and optimizer state: the eager twin, which runs the default launches)
    for m in (m_e, m_g):
        m.set_cond_dropout(0.0)
    (le3, me3), (lg3, mg3) = _steps(dev, m_e, tr_e, 3, first=6), _steps(dev, m_g, tr_g, 3, first=6)
    assert tr_g.graph_steps == 5                                         # two eager sightings again, then a replay
    assert me3 == mg3 == [None] * 3
    assert all(torch.equal(a, b) for a, b in zip(le3, lg3))
    assert all(torch.equal(a, b) for a, b in zip(m_e.parameters(), m_g.parameters()))


def test_trainer_without_dropout_after_set_cond_dropout_zero(dev):
    """set_cond_dropout(0.0) before the first step is a Trainer that never had dropout, bit for bit, replay included."""
    m_a, tr_a = _trainer(dev, True, p=0.5)
    m_a.set_cond_dropout(0.0)
    from view_fusion_amd import train
    m_b = _model(dev)
    tr_b = train.Trainer(m_b, lr_warmup=1, graph=True, seed=TSEED)
    tr_b.it = 0
    (la, ma), (lb, mb) = _steps(dev, m_a, tr_a, 3), _steps(dev, m_b, tr_b, 3)
    assert ma == mb == [None] * 3 and tr_a.graph_steps == tr_b.graph_steps == 1
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    assert all(torch.equal(a, b) for a, b in zip(m_a.parameters(), m_b.parameters()))


def test_trainer_accum_steps_see_the_same_masks(dev):
    m1, tr1 = _trainer(dev, False)
    m2, tr2 = _trainer(dev, False, accum_steps=2)
    seen = []
    m2.register_forward_hook(lambda mod, args, out: seen.append(mod.last_cond_drop.cpu().numpy().astype(bool)))
    batch = _batch(dev, TB, TVC)
    l1, l2 = float(tr1.step(batch)), float(tr2.step(batch))
    whole = m1.last_cond_drop.cpu().numpy().astype(bool)
    assert len(seen) == 2 and np.array_equal(np.concatenate(seen), whole)
    assert np.array_equal(whole, guidance_ref.cond_drop(TSEED, np.arange(TB, 2 * TB), 0.5)) and whole.any() and not whole.all()
    print(f"accum_steps=2 loss {l2:.9g}  undivided {l1:.9g}  |diff| / loss {abs(l2 - l1) / abs(l1):.2e}")
    # the same samples with the same masks through the same fp32 network, summed in another order (and, the stacked batch
    # being half as large, possibly by other kernels): 1e-5 relative is what smoke() allows a training loss against float64
    assert abs(l2 - l1) <= 1e-5 * abs(l1)


# ---- 7. drivers ---------------------------------------------------------------------------------------------------------
def test_drivers_take_the_scale(vf, dev):
    from view_fusion_amd import drivers
    g = torch.Generator().manual_seed(701)
    full = dict(target=torch.rand(3, 3, HW, HW, generator=g).to(dev), cond=torch.rand(3, 6, 3, HW, HW, generator=g).to(dev),
                angle=torch.rand(3, 1, generator=g).to(dev), view_count=torch.tensor([2, 6, 1]), ids=torch.tensor([11, 5, 8]))
    a = drivers.evaluate(vf, [full], seed=21, sample_steps=3, guidance=3.0)
    b = drivers.evaluate(vf, [full], seed=21, sample_steps=3)
    assert torch.isfinite(a["psnr"]) and torch.isfinite(b["psnr"]) and float(a["psnr"]) != float(b["psnr"])
    first = torch.rand(2, 3, HW, HW, generator=g).to(dev)
    r = drivers.autoregressive_rollout(vf, first, steps=2, sample_steps=2, seed=4, guidance=3.0)
    assert r.shape == (2, 2, 3, HW, HW) and torch.isfinite(r).all()
    assert not torch.equal(r, drivers.autoregressive_rollout(vf, first, steps=2, sample_steps=2, seed=4))
    cond23 = torch.rand(2, 23, 3, HW, HW, generator=g).to(dev)
    ang = torch.rand(2, 1, generator=g).to(dev)
    kw = dict(view_count=torch.tensor([7, 9]), sample_steps=2, seed=4)
    ex, logit_arr, *_ = drivers.extrapolate(vf, cond23, ang, guidance=3.0, **kw)
    assert torch.isfinite(ex).all() and logit_arr.shape[0] == 16 and not torch.equal(ex, drivers.extrapolate(vf, cond23, ang, **kw)[0])
    views = torch.rand(24, 3, HW, HW, generator=g).to(dev)
    fr, *_ = drivers.orbit_frames(vf, views, sample_steps=2, seed=4, guidance=3.0)
    assert fr.shape[0] == 24 and torch.isfinite(fr).all()
    assert not torch.equal(fr, drivers.orbit_frames(vf, views, sample_steps=2, seed=4)[0])
