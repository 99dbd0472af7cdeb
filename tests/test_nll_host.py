"""The variational bound on the host (the head of csrc/diffusion.hip holds the definition, csrc/vlb.h the arithmetic):
schedule.nll_tables against the schedule buffers, the sampler tables and a direct float64 formula; the library's host
mirror of one term (the function the kernel runs) against the float64 restatement tests/nll_ref.py on conditioned
inputs, and against that restatement's float32 run on saturated ones; closed forms with an "oracle network"; the new
entry points' declarations; the refusals that need no device.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import nll_ref
from conftest import ROOT, TINY

SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
T = SCHED["num_timesteps"]
NEW = ("vf_nll_noisy", "vf_nll_terms", "vf_nll_prior", "vf_nll_terms_host")
PREDS = ("eps", "v", "x0")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from view_fusion_amd import _lib
    return _lib.load()


def _tabs32(prediction="eps", tau=None, fixed_variance="small", sched=SCHED):
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**sched)
    tab = {k: v.astype(np.float32) for k, v in schedule.nll_tables(betas, tau, prediction, fixed_variance).items()}
    gam = schedule.schedule_tensors(betas, "cpu")["gammas"].numpy()
    tau = np.arange(len(betas)) if tau is None else np.asarray(tau)
    return tab, gam, tau


# ---- tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", [SCHED, dict(schedule="cosine", num_timesteps=50),
                                   dict(schedule="linear", num_timesteps=1000, linear_start=1e-6, linear_end=1e-2)])
def test_tables_on_the_full_chain_are_the_buffers(sched):
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**sched)
    bufs = schedule.schedule_tensors(betas, "cpu")
    for tau in (None, np.arange(len(betas))):
        tab = schedule.nll_tables(betas, tau)
        assert all(tab[k].dtype == np.float64 and tab[k].shape == (len(betas),) for k in ("a", "b", "c0", "hi", "lo"))
        f32 = {k: v.astype(np.float32) for k, v in tab.items()}
        assert np.array_equal(f32["c0"][1:], bufs["posterior_mean_coef1"].numpy()[1:])               # value for value
        assert np.array_equal(f32["lo"][1:], bufs["posterior_log_variance_clipped"].numpy()[1:])
        assert np.array_equal(tab["hi"][1:], np.log(np.asarray(betas, dtype=np.float64))[1:])
        assert np.array_equal(f32["a"], bufs["sqrt_recip_gammas"].numpy())
        assert np.array_equal(f32["b"], bufs["sqrt_recipm1_gammas"].numpy())
        # the decoder row: not the 1e-20 clipping
        gam = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
        assert tab["lo"][0] == tab["lo"][1] and tab["hi"][0] == np.log(1.0 - gam[0]) and tab["lo"][0] > np.log(1e-19)
    large = schedule.nll_tables(betas, None, "eps", "large")
    assert large["hi"][0] == large["lo"][0] == tab["lo"][0] and np.array_equal(large["hi"][1:], tab["hi"][1:])
    with pytest.raises(ValueError):
        schedule.nll_tables(betas, None, "eps", "medium")
    with pytest.raises(ValueError):
        schedule.nll_tables(betas, None, "noise")


@pytest.mark.parametrize("K", [1, 2, 5, 7, 19])
@pytest.mark.parametrize("prediction", PREDS)
def test_tables_on_a_strided_chain(K, prediction):
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**SCHED)
    tau = schedule.sample_timesteps(T, K)
    tab = schedule.nll_tables(betas, tau, prediction)
    want = nll_ref.tables(betas, tau, prediction)
    for k in ("a", "b", "c0", "hi", "lo"):
        assert tab[k].shape == (K,) and np.allclose(tab[k], want[k], rtol=1e-13, atol=0), k
    c0 = schedule.sampler_tables(betas, tau, "ddim", 1.0, prediction)["c0"]
    assert np.all(np.abs(tab["c0"] - c0) <= 1e-12 * np.abs(c0))
    if K == 1:
        assert tab["lo"][0] == tab["hi"][0]                       # a one-step chain: lo_dec = hi_dec
    else:
        assert tab["lo"][0] == tab["lo"][1]
        hi, lo = schedule.variance_tables(betas, tau)
        assert np.array_equal(tab["hi"][1:], hi[1:]) and np.array_equal(tab["lo"][1:], lo[1:])


def test_zero_terminal_snr():
    from view_fusion_amd import schedule
    betas = schedule.make_beta_schedule(**SCHED, zero_terminal_snr=True)
    for tau in (None, schedule.sample_timesteps(T, 4)):
        with pytest.raises(ValueError):
            schedule.nll_tables(betas, tau, "eps")
        for prediction in ("v", "x0"):
            tab = schedule.nll_tables(betas, tau, prediction)
            assert all(np.isfinite(v).all() for v in tab.values()), (prediction, tab)
    gam = np.cumprod(1.0 - betas)
    assert gam[-1] == 0.0
    y_0 = np.random.default_rng(0).uniform(-1, 1, (2, 3, 4, 4))
    for dt in (np.float64, np.float32):
        assert np.all(nll_ref.prior(y_0, gam[-1], dt) == 0)      # exactly 0


# ---- the host mirror against float64 ----------------------------------------------------------------------------------------
HOST_CASES = [(learned, decoder, large) for learned in (False, True) for decoder in (False, True)
              for large in ((False, True) if not learned else (False,))]


def _host_term(case, row, learned, decoder, large, clip=True, weighting=True, vc=(1, 3, 2)):
    """The host mirror on the float32 composition of the case's views (the composition is the kernel's, not the
    mirror's): per element term and (y0 - y_0)^2."""
    from view_fusion_amd import ops
    e_b, o_b = nll_ref.compose(case["out"], vc, weighting, np.float32)
    n = e_b.size
    full = lambda v: np.full(n, v, dtype=np.float32)               # noqa: E731
    t, sq = ops.nll_terms_host(e_b.ravel(), None if o_b is None or not learned else o_b.ravel(), case["y_k"].ravel(),
                               case["y_0"].ravel(), *(full(v) for v in row), learned=learned, decoder=decoder, large=large,
                               clip=clip)
    return t.numpy().reshape(len(vc), -1), sq.numpy().reshape(len(vc), -1)


@pytest.mark.parametrize("prediction", PREDS)
@pytest.mark.parametrize("learned,decoder,large", HOST_CASES)
def test_host_mirror_against_float64(lib, prediction, learned, decoder, large):
    """Tolerance: the float32 run of the restatement on the same inputs measures its own distance from float64; the mirror
    may be 4 x as far (expf / tanhf / logf against numpy's, the header's fixed operation order), per quantity over the
    case's samples; no other floor (every measured floor is nonzero)."""
    tab, gam, tau = _tabs32(prediction, fixed_variance="large" if large else "small")
    vc = (1, 3, 2)
    for k in ((0,) if decoder else (1, 7, T - 1)):
        case = nll_ref.conditioned_case(tab, gam, tau, k, (12, 20), vc, True, learned)
        args = (case["out"], vc, True, case["y_k"], case["y_0"], case["row"])
        r64 = nll_ref.term(*args, learned=learned, decoder=decoder, large=large, dt=np.float64)
        r32 = nll_ref.term(*args, learned=learned, decoder=decoder, large=large, dt=np.float32)
        if decoder:
            assert r64["mass"].min() >= 1e-3, r64["mass"].min()      # every element, nothing left out
        t, sq = _host_term(case, case["row"], learned, decoder, large)
        for name, got, w64, w32 in (("vb", t.mean(axis=1), r64["vb"], r32["vb"]),
                                    ("x0_mse", sq.mean(axis=1), r64["x0_mse"], r32["x0_mse"])):
            e32 = np.abs(w32.astype(np.float64) - w64) / np.abs(w64)
            e = np.abs(got.astype(np.float64) - w64) / np.abs(w64)
            print(f"{prediction} lv={learned} dec={decoder} large={large} k={k} {name}: f64 {w64}  mirror rel {e.max():.2e}  "
                  f"fp32 restatement rel {e32.max():.2e}")
            assert e32.max() > 0 and np.all(e <= 4.0 * e32.max()), (name, k, e, e32)
    assert lib.vf_nll_terms_host(None, None, None, None, None, None, None, None, None, 1, 0, 1, 1, None, None, 0) != 0
    # null pointers are refused, not read: every operand missing, then the raw variance alone (lv)
    assert lib.vf_nll_terms_host(None, None, None, None, None, None, None, None, None, 0, 0, 0, 1, None, None, 1) != 0
    one = [np.zeros(1, dtype=np.float32) for _ in range(10)]
    ptr = [x.ctypes.data for x in one]
    assert lib.vf_nll_terms_host(ptr[0], None, *ptr[1:8], 0, 0, 0, 1, ptr[8], ptr[9], 1) == 0
    assert lib.vf_nll_terms_host(ptr[0], None, *ptr[1:8], 1, 0, 0, 1, ptr[8], ptr[9], 1) != 0
    assert lib.vf_nll_terms_host(ptr[0], None, *ptr[1:8], 0, 0, 0, 1, ptr[8], None, 1) != 0
    assert lib.vf_nll_terms_host(None, None, None, None, None, None, None, None, None, 0, 0, 0, 1, None, None, 0) == 0


@pytest.mark.parametrize("edge", [-1.0, 1.0, 0.25])
def test_saturated_inputs_hit_the_clamp_like_the_float32_restatement(lib, edge):
    """A prediction many sd away, y_0 inside and at both edges: the float32 restatement and the mirror both take
    log(1e-12); one part in 1e6 covers logf against numpy's log."""
    from view_fusion_amd import ops
    tab, gam, tau = _tabs32("x0")
    row = tuple(tab[n][0] for n in ("a", "b", "c0", "hi", "lo"))
    n = 64
    y_0 = np.full(n, edge, dtype=np.float32)
    out = np.full(n, -edge if abs(edge) == 1 else -0.9, dtype=np.float32)     # x0: a = 0, b = -1, so y0 == out
    y_k = np.zeros(n, dtype=np.float32)
    full = lambda v: np.full(n, v, dtype=np.float32)               # noqa: E731
    t, _ = ops.nll_terms_host(out, None, y_k, y_0, *(full(v) for v in row), decoder=True)
    ref32, mass = nll_ref.decoder_parts(y_0, out, full(row[4]), np.float32)
    assert ref32.dtype == np.float32 and np.all(mass < 1e-12)
    assert np.allclose(t.numpy(), ref32, rtol=1e-6, atol=0)
    assert np.allclose(t.numpy(), -np.log2(1e-12), rtol=1e-6)


# ---- closed forms with an oracle network -------------------------------------------------------------------------------------
def _oracle_case(prediction, k, learned, o_value=0.0, fixed_variance="small"):
    """out = the exact target in every view (y0 == y_0 up to fp32 rounding), variance channels = o_value."""
    tab, gam, tau = _tabs32(prediction, fixed_variance=fixed_variance)
    row = tuple(tab[n][k] for n in ("a", "b", "c0", "hi", "lo"))
    g = np.random.default_rng(3)
    y_0 = g.uniform(-0.95, 0.95, 512).astype(np.float32)
    y_k = nll_ref.noisy(y_0.reshape(1, 1, 1, -1), g.standard_normal(512).reshape(1, 1, 1, -1), gam[k], np.float64).ravel()
    out = nll_ref.exact_output(y_k, y_0, row)
    return row, out.astype(np.float32), y_k.astype(np.float32), y_0, np.full(512, o_value, dtype=np.float32)


@pytest.mark.parametrize("prediction", PREDS)
def test_closed_forms(lib, prediction):
    from view_fusion_amd import ops
    full = lambda v: np.full(512, v, dtype=np.float32)              # noqa: E731
    for k in (1, 7, T - 1):
        row, out, y_k, y_0, o = _oracle_case(prediction, k, False)
        a, b, c0, hi, lo = (np.float64(v) for v in row)
        # the residual an fp32 "exact" output leaves: y0 - y_0 is rounding noise of size ~ eps (|a y_k| + |b out|)
        slack = 0.5 * (c0 * 4e-7 * (np.abs(a * y_k) + np.abs(b * out) + 1).max()) ** 2 * np.exp(-lo) / np.log(2.0)
        t, _ = ops.nll_terms_host(out, None, y_k, y_0, *(full(v) for v in row))
        assert np.all(t.numpy() >= 0) and t.numpy().max() <= slack, (k, t.numpy().max(), slack)   # fixed-small: 0
        # o = -1: v = 0, lp = lo exactly -> 0
        t, _ = ops.nll_terms_host(out, full(-1.0), y_k, y_0, *(full(v) for v in row), learned=True)
        assert t.numpy().max() <= slack
        # o = +1: v = 1, lp = hi exactly
        t, _ = ops.nll_terms_host(out, full(1.0), y_k, y_0, *(full(v) for v in row), learned=True)
        want = 0.5 * (-1.0 + hi - lo + np.exp(lo - hi)) / np.log(2.0)
        slack_hi = slack * np.exp(lo - hi) + 4e-6 * max(abs(want), abs(hi - lo))
        assert np.all(np.abs(t.numpy() - want) <= slack_hi), (k, want, t.numpy()[:4])
        # fixed-large is the same number
        rowL = row
        tL, _ = ops.nll_terms_host(out, None, y_k, y_0, *(full(v) for v in rowL), large=True)
        assert np.array_equal(tL.numpy(), t.numpy())
    # the decoder with y0 == y_0 inside the image range: -log2(Phi(delta / sd) - Phi(-delta / sd))
    row, out, y_k, y_0, _ = _oracle_case(prediction, 0, False)
    sd = np.exp(0.5 * np.float64(row[4]))
    want = -np.log2(nll_ref.cdf(nll_ref.DELTA / sd) - nll_ref.cdf(-nll_ref.DELTA / sd))
    t, sq = ops.nll_terms_host(out, None, y_k, y_0, *(full(v) for v in row), decoder=True)
    resid = np.sqrt(sq.numpy().astype(np.float64)).max() / sd        # how far the fp32 "exact" output is from exact, in sd
    assert np.all(np.abs(t.numpy() - want) <= (resid ** 2 + 1e-5) * max(want, 1.0)), (want, t.numpy()[:4], resid)


# ---- declarations ------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_typed(lib):
    from view_fusion_amd import _lib
    from view_fusion_amd.ops import core
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    source = open(os.path.join(ROOT, "view_fusion_amd", "csrc", "diffusion.hip")).read()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/vf_hip.h"
        d = re.search(r"\bint\s+" + name + r"\s*\(([^{]*?)\)\s*\{", source, re.S)
        assert d, f"{name} is not defined in csrc/diffusion.hip"
        assert len(m.group(1).split(",")) == len(d.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
        assert hasattr(lib, name)
        if not name.endswith("_host"):
            assert core._CALL_KIND[name] == "diffusion"
    spec = open(os.path.join(ROOT, "view_fusion_amd", "csrc", "vlb.h")).read()
    assert "vf_nll_cdf" in spec and "vf_nll_decoder" in spec
    rng = open(os.path.join(ROOT, "view_fusion_amd", "csrc", "rng.h")).read()
    assert "kind 6" in rng and "VF_RNG_NLL_NOISE = 6" in rng
    # argument checks that need no device: B <= 0 returns 0 first, then null pointers / HW % 4
    assert lib.vf_nll_terms(*([None] * 14), 0, 6, 16, 4, 1, 1, 0, 0, 0, None) == 0
    assert lib.vf_nll_prior(None, None, None, None, 0, 16, 4, None) == 0
    assert lib.vf_nll_noisy(None, None, 0, None, None, None, None, None, 0, 16, 4, 4, None) == 0
    assert lib.vf_nll_terms(*([None] * 14), 2, 6, 16, 4, 1, 1, 0, 0, 0, None) != 0
    assert lib.vf_nll_prior(None, None, None, None, 2, 16, 4, None) != 0
    assert lib.vf_nll_noisy(None, None, 0, None, None, None, None, None, 2, 16, 4, 4, None) != 0


# ---- refusals that need no device ----------------------------------------------------------------------------------------------
def _cpu_model(cfg=TINY):
    from view_fusion_amd import UNet, ViewFusion
    vf = ViewFusion(UNet(**cfg), {"train": dict(SCHED)}, True, True)
    vf.set_new_noise_schedule(device=torch.device("cpu"), phase="train")
    return vf


def test_refusals_before_anything_touches_the_library():
    from view_fusion_amd import _lib, drivers
    vf = _cpu_model()
    y_cond, angle, y_0 = torch.rand(2, 2, 3, 16, 16), torch.rand(2, 1), torch.rand(2, 3, 16, 16)
    n0 = _lib.N_CALLS
    for kw in (dict(guidance=2.0), dict(threshold=0.9), dict(guidance_rescale=0.5), dict(fixed_variance="medium"), {}):
        with pytest.raises(ValueError):                              # ({}: a CPU model)
            vf.bound_terms(y_cond, [2, 2], angle, y_0, **kw)
    vf.set_self_cond(0.5)
    with pytest.raises(ValueError, match="self-conditioned"):
        vf.bound_terms(y_cond, [2, 2], angle, y_0)
    vf.set_self_cond(None)
    nine = _cpu_model(dict(TINY, out_channel=9))
    nine.set_learned_variance(1e-3)
    with pytest.raises(ValueError, match="large"):
        nine.bound_terms(y_cond, [2, 2], angle, y_0, fixed_variance="large")
    with pytest.raises(ValueError):
        drivers.evaluate(vf, [], nll=True, guidance=2.0)
    cpu_batch = [dict(target=y_0, cond=y_cond, angle=angle, view_count=torch.tensor([2, 2]))]
    with pytest.raises(ValueError, match="GPU"):                     # before the first generate()
        drivers.evaluate(vf, cpu_batch, nll=True)
    vf.set_self_cond(0.5)
    with pytest.raises(ValueError, match="self-conditioned"):
        drivers.evaluate(vf, cpu_batch, nll=True)
    vf.set_self_cond(None)
    assert _lib.N_CALLS == n0
