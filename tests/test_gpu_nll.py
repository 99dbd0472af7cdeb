"""The terms of the variational bound on the GPU, through the C ABI (ops.nll_terms / nll_prior / nll_noisy; the kernels
nll_term_kernel<LV, DEC>, nll_prior_kernel, nll_finish_kernel and nll_noisy_kernel<RNG> of csrc/diffusion.hip; definition
at the head of that file, arithmetic in csrc/vlb.h) against the float64 restatement tests/nll_ref.py.

  1. every instantiation of the term kernel against float64: eps / v / x0 x softmax / mean (x small / large for a fixed
     variance), B = 3 with ragged view counts (1, 3, 2), at the smallest shapes at which this geometry can go wrong --
     2x2 (3 float4: one partial wave), 8x8 (fewer float4 than one workgroup), 12x20 (a channel boundary inside a chunk,
     HW % 256 != 0), 32x32 (several chunks) -- on the conditioned inputs of nll_ref.conditioned_case (the float64 side
     asserts that every decoder element keeps a probability mass >= 1e-3; nothing is left out).
     Tolerance: no number fixed in advance.  The float32 run of the restatement on the same inputs measures the formulas'
     own rounding floor against the float64 run; the maximum of that over the instantiation's cases, times 4, is what the
     device gets (it reduces 256-wide in another order and uses the device expf / tanhf / logf).  No other floor: every
     measured floor is nonzero.  The grid-stride and the prior test take the floor per quantity (and per instantiation).
  2. the prior term likewise; exactly 0 where gammas[T-1] = 0.
  3. vb / x0_mse are the same bits on two runs, and for B = 3 against the same samples one at a time.
  4. the seeded noisy target: the Philox words of kind 6 at step tau[k] are rng_ref.words' bit for bit, and the normals the
     kernel draws are ops.randn_ids' of those counters bit for bit (one device function); the normals are those of kind 6
     at step tau[k] (within rng_ref's bound of the float64 restatement: Box-Muller on the device's logf / cosf is not numpy's, as tests/test_gpu_rng.py explains -- measured,
     22 ... 29 % of the device's normals differ from the float32 restatement's in their last bits), y_k is the
     restatement's float32 arithmetic on those normals bit for bit, and a sample's target does not depend on its row or on
     the rest of the batch, bit for bit; an injected noise wins.
Figures are printed before the assertions (run with -s); profiles/nll.md records them."""
import numpy as np
import pytest
import torch

import nll_ref
import rng_ref

pytestmark = pytest.mark.gpu
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
T = SCHED["num_timesteps"]
VC = (1, 3, 2)
SHAPES = [(2, 2), (8, 8), (12, 20), (32, 32)]
PREDS = ("eps", "v", "x0")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


_TABS = {}


def _tabs(prediction, fixed_variance="small", steps=None):
    """The fp32 table values the device reads, on the host, with the fp32 gammas and the chain."""
    key = (prediction, fixed_variance, steps)
    if key not in _TABS:
        from view_fusion_amd import schedule
        betas = schedule.make_beta_schedule(**SCHED)
        tau = np.arange(T) if steps is None else schedule.sample_timesteps(T, steps)
        tab = {k: v.astype(np.float32) for k, v in schedule.nll_tables(betas, tau, prediction, fixed_variance).items()}
        _TABS[key] = (tab, schedule.schedule_tensors(betas, "cpu")["gammas"].numpy(), tau)
    return _TABS[key]


def _dv(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _run_term(dev, tab, case, k, vc, weighting, learned, decoder, large, clip=True, rows=None):
    """ops.nll_terms on one case (rows: the samples to run, default all) -> (vb, x0_mse) float32 (B,) of column k."""
    from view_fusion_amd import ops
    rows = list(range(len(vc))) if rows is None else rows
    off_h = np.concatenate([[0], np.cumsum(vc)])
    views = np.concatenate([np.arange(off_h[i], off_h[i + 1]) for i in rows])
    sub = [vc[i] for i in rows]
    off, _, _ = ops.view_offsets(sub, dev)
    tabs = {n: _dv(dev, tab[n]) for n in ("a", "b", "c0", "hi", "lo")}
    kidx = torch.full((len(rows),), k, device=dev, dtype=torch.int64)
    vb, mse = ops.nll_terms(_dv(dev, case["out"][views]), off, _dv(dev, case["y_k"][rows]), _dv(dev, case["y_0"][rows]), kidx,
                            tabs, len(rows), weighting, learned=learned, decoder=decoder, large=large, clip=clip)
    others = [j for j in range(vb.shape[1]) if j != k]
    assert not vb[:, others].any() and not mse[:, others].any()     # only column k is written
    return vb[:, k].cpu().numpy(), mse[:, k].cpu().numpy()


# ---- 1. the term kernel against float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("learned,decoder", [(False, False), (False, True), (True, False), (True, True)])
def test_terms_against_float64(dev, learned, decoder):
    cases = []
    for prediction in PREDS:
        for large in ((False,) if learned else (False, True)):
            tab, gam, tau = _tabs(prediction, "large" if large else "small")
            for weighting in (True, False):
                for hw in SHAPES:
                    for k in ((0,) if decoder else (1, T - 1)):
                        for clip in ((True, False) if hw == (8, 8) else (True,)):
                            cases.append((prediction, large, weighting, hw, k, clip, tab, gam, tau))
    rec = []
    for prediction, large, weighting, hw, k, clip, tab, gam, tau in cases:
        n4 = 3 * hw[0] * hw[1] // 4
        assert {(2, 2): n4 == 3, (8, 8): n4 < 256, (12, 20): n4 % 256 != 0 and (hw[0] * hw[1]) % 256 != 0,
                (32, 32): n4 > 2 * 256}[hw]
        case = nll_ref.conditioned_case(tab, gam, tau, k, hw, VC, weighting, learned)
        args = (case["out"], VC, weighting, case["y_k"], case["y_0"], case["row"])
        kw = dict(learned=learned, decoder=decoder, large=large, clip=clip)
        r64 = nll_ref.term(*args, **kw, dt=np.float64)
        r32 = nll_ref.term(*args, **kw, dt=np.float32)
        if decoder:
            assert r64["mass"].min() >= 1e-3, (prediction, hw, r64["mass"].min())
        vb, mse = _run_term(dev, tab, case, k, VC, weighting, learned, decoder, large, clip)
        for name, got, w64, w32 in (("vb", vb, r64["vb"], r32["vb"]), ("x0_mse", mse, r64["x0_mse"], r32["x0_mse"])):
            e32 = float((np.abs(w32.astype(np.float64) - w64) / np.abs(w64)).max())
            e = float((np.abs(got.astype(np.float64) - w64) / np.abs(w64)).max())
            rec.append((name, prediction, large, weighting, hw, k, clip, e, e32))
    for name in ("vb", "x0_mse"):
        mine = [r for r in rec if r[0] == name]
        floor = max(r[8] for r in mine)
        tol = 4.0 * floor
        assert floor > 0
        worst = max(mine, key=lambda r: r[7])
        print(f"nll_term_kernel<LV={learned}, DEC={decoder}> {name}: {len(mine)} cases, fp32 restatement floor {floor:.2e}, "
              f"tolerance {tol:.2e}, device worst {worst[7]:.2e} at {worst[1:7]}")
        bad = [r for r in mine if not r[7] <= tol]
        assert not bad, bad


def test_grid_stride_loop(dev):
    """128x192 at B = 1: 3 HW / 4 = 18432 float4 > 64 workgroups x 256, so every thread takes a second trip and all 64
    partials are in use (the other shapes never stride)."""
    rec = []
    for learned, decoder, k in ((False, False, 7), (True, True, 0)):
        tab, gam, tau = _tabs("v")
        case = nll_ref.conditioned_case(tab, gam, tau, k, (128, 192), (2,), True, learned)
        args = (case["out"], (2,), True, case["y_k"], case["y_0"], case["row"])
        r64 = nll_ref.term(*args, learned=learned, decoder=decoder, dt=np.float64)
        r32 = nll_ref.term(*args, learned=learned, decoder=decoder, dt=np.float32)
        assert not decoder or r64["mass"].min() >= 1e-3
        vb, mse = _run_term(dev, tab, case, k, (2,), True, learned, decoder, False)
        for name, got in (("vb", vb), ("x0_mse", mse)):
            e32 = float(abs(float(r32[name][0]) - r64[name][0]) / r64[name][0])
            e = float(abs(float(got[0]) - r64[name][0]) / r64[name][0])
            print(f"128x192 LV={learned} DEC={decoder} {name}: device {e:.2e}  fp32 restatement {e32:.2e}")
            rec.append((e, e32))
    assert all(0 < r[1] and r[0] <= 4.0 * r[1] for r in rec), rec        # each quantity of each instantiation on its own


# ---- 2. the prior ----------------------------------------------------------------------------------------------------------------
def test_prior_against_float64(dev):
    from view_fusion_amd import ops, schedule
    rec = []
    for zero in (False, True):
        betas = schedule.make_beta_schedule(**SCHED, zero_terminal_snr=zero)
        gam = schedule.schedule_tensors(betas, "cpu")["gammas"]
        for hw in SHAPES:
            y_0 = np.random.default_rng(hw[0]).uniform(-1, 1, (3, 3) + hw).astype(np.float32)
            got = ops.nll_prior(_dv(dev, y_0), gam.to(dev)).cpu().numpy()
            w64, w32 = nll_ref.prior(y_0, gam.numpy()[-1]), nll_ref.prior(y_0, gam.numpy()[-1], np.float32)
            if zero:
                assert gam[-1] == 0 and np.all(got == 0) and np.all(w64 == 0)
                continue
            rec.append((hw, float((np.abs(got - w64) / w64).max()), float((np.abs(w32 - w64) / w64).max())))
    floor = max(r[2] for r in rec)
    print(f"nll_prior_kernel: fp32 restatement floor {floor:.2e}, device worst {max(r[1] for r in rec):.2e}")
    assert floor > 0 and all(r[1] <= 4.0 * floor for r in rec), rec


# ---- 3. the same bits on every run and for every batch ------------------------------------------------------------------------------
@pytest.mark.parametrize("learned,decoder", [(False, False), (True, True)])
def test_bits_do_not_depend_on_the_run_or_the_batch(dev, learned, decoder):
    tab, gam, tau = _tabs("eps")
    k = 0 if decoder else 7
    for hw in ((12, 20), (32, 32)):
        case = nll_ref.conditioned_case(tab, gam, tau, k, hw, VC, True, learned)
        one = _run_term(dev, tab, case, k, VC, True, learned, decoder, False)
        two = _run_term(dev, tab, case, k, VC, True, learned, decoder, False)
        assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
        for i in range(len(VC)):
            alone = _run_term(dev, tab, case, k, VC, True, learned, decoder, False, rows=[i])
            assert alone[0][0] == one[0][i] and alone[1][0] == one[1][i], (hw, i)
        back = _run_term(dev, tab, case, k, VC, True, learned, decoder, False, rows=[2, 0, 1])
        assert np.array_equal(back[0], one[0][[2, 0, 1]]) and np.array_equal(back[1], one[1][[2, 0, 1]])


# ---- 4. the noisy target ---------------------------------------------------------------------------------------------------------------
def test_seeded_noisy_target(dev):
    from view_fusion_amd import ops, schedule
    betas = schedule.make_beta_schedule(**SCHED)
    gam = schedule.schedule_tensors(betas, "cpu")["gammas"]
    seed, ids = 0x1234_5678_9ABC_DEF0, np.array([5, 2 ** 40 + 3, 0], dtype=np.int64)
    for steps, hw in ((None, (12, 20)), (4, (32, 32)), (None, (2, 2))):
        tau = np.arange(T) if steps is None else schedule.sample_timesteps(T, steps)
        K = len(tau)
        tau_d = _dv(dev, tau.astype(np.int64))
        y_0 = np.random.default_rng(1).uniform(-1, 1, (3, 3) + hw).astype(np.float32)
        for k in (0, K // 2, K - 1):
            kidx = torch.full((3,), k, device=dev, dtype=torch.int64)
            y_k = ops.nll_noisy(_dv(dev, y_0), kidx, tau_d, gam.to(dev), seed=seed, ids=_dv(dev, ids)).cpu().numpy()
            # the device's own normals: the same launch at a level of 0 on a zero target (sqrt(0) 0 + sqrt(1) n = n exactly)
            n_dev = ops.nll_noisy(torch.zeros(3, 3, *hw, device=dev), kidx, tau_d, torch.zeros(T, device=dev), seed=seed,
                                  ids=_dv(dev, ids)).cpu().numpy()
            # ... come from the kind-6 words of (seed, id, step = tau[k], block), bit for bit ...
            nb = n_dev[0].size // 4
            w_dev = ops.philox_ids(seed, _dv(dev, ids), nll_ref.KIND_NLL_NOISE, int(tau[k]), 4 * nb).cpu().numpy()
            w_ref = rng_ref.words(seed, ids, nll_ref.KIND_NLL_NOISE, int(tau[k]), nb).reshape(3, -1)
            assert np.array_equal(w_dev.view(np.uint32).astype(np.uint64), w_ref)
            r_dev = ops.randn_ids(seed, _dv(dev, ids), nll_ref.KIND_NLL_NOISE, int(tau[k]), (3,) + hw).cpu().numpy()
            assert np.array_equal(n_dev, r_dev)
            # ... and are the kind-6 normals of the float64 restatement within its bound ...
            n64 = nll_ref.seeded_normals(seed, ids, int(tau[k]), (3,) + hw)
            _, e32, bound = rng_ref.bound(seed, ids, nll_ref.KIND_NLL_NOISE, int(tau[k]), 3 * hw[0] * hw[1])
            err = float(np.abs(n_dev.astype(np.float64) - n64).max())
            n32 = nll_ref.seeded_normals(seed, ids, int(tau[k]), (3,) + hw, np.float32)
            print(f"K {K} {hw} k {k} (t {int(tau[k])}): normals max|device - float64| {err:.2e}  fp32 restatement {e32:.2e}  "
                  f"elements whose bits differ from the fp32 restatement's: {int((n_dev != n32).sum())} of {n32.size}")
            assert err <= bound
            # ... and of no other kind or step
            assert np.abs(n_dev - rng_ref.normal(seed, ids, 3, int(tau[k]), n_dev[0].size).reshape(n_dev.shape)).max() > 1
            # y_k is the restatement's float32 arithmetic on those normals, bit for bit
            assert np.array_equal(y_k, nll_ref.noisy(y_0, n_dev, gam.numpy()[tau[k]], np.float32))
            # a sample's target depends on (seed, id, step) alone: another order, and each sample alone
            perm = [2, 0, 1]
            y_p = ops.nll_noisy(_dv(dev, y_0[perm]), kidx, tau_d, gam.to(dev), seed=seed, ids=_dv(dev, ids[perm])).cpu().numpy()
            assert np.array_equal(y_p, y_k[perm])
            for i in range(3):
                y_i = ops.nll_noisy(_dv(dev, y_0[i:i + 1]), kidx[:1], tau_d, gam.to(dev), seed=seed, ids=_dv(dev, ids[i:i + 1]))
                assert np.array_equal(y_i.cpu().numpy()[0], y_k[i])
            # an injected draw wins
            noise = np.random.default_rng(2).standard_normal((3, K, 3) + hw).astype(np.float32)
            y_n = ops.nll_noisy(_dv(dev, y_0), kidx, tau_d, gam.to(dev), noise=_dv(dev, noise), seed=seed,
                                ids=_dv(dev, ids)).cpu().numpy()
            assert np.array_equal(y_n, nll_ref.noisy(y_0, noise[:, k], gam.numpy()[tau[k]], np.float32))
    with pytest.raises(ValueError):
        ops.nll_noisy(_dv(dev, y_0), kidx, tau_d, gam.to(dev))
