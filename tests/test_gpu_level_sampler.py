"""Loss-aware noise-level sampling on the GPU (ops.draw_level / level_stats / compose_loss(sample_scale=),
ViewFusion.set_level_sampler, train.Trainer; draw_level_kernel, level_stats_kernel and compose_loss_finish_kernel's scale
of csrc/diffusion.hip, specification in csrc/level_sampler.h), against tests/level_sampler_ref.py:

  1. the draw kernel, bitwise in t / u / iw, seeded and from words, B = 1000, skewed tables at (T, K) = (20, 4), (2000, 64);
  2. the statistics + table kernel: B = 70 samples (more than the 64 threads of the finish kernel it follows), K = 100
     bins, T = 401, two calls (first update, EMA update, empty bins, more than one sample per bin), one NaN loss;
  3. the warm-up is the uniform path, bit for bit; 4. compose_loss(sample_scale=) against float64;
  5. / 6. model level: the exact uniform table, and a skewed table against weighted single-sample runs;
  7. Trainer: replay == eager through the flip of `ready`, accum_steps, set_level_sampler after capture, checkpoints;
  8. set_level_sampler(None) leaves the default step's launches and bits alone;
  and the unseeded path: one randint word per sample where t is drawn today.
Figures are printed before the assertions (run with -s); profiles/level_sampler.md records them."""
import ctypes

import numpy as np
import pytest
import torch

import level_sampler_ref as lsr
import loss_ref
import rng_ref
from conftest import TINY

pytestmark = pytest.mark.gpu
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
Q4 = [1.0, 50.0, 0.01, 8.0]
_Q64 = np.exp(np.linspace(-6.0, 3.0, 64)) * (1.0 + 0.5 * np.sin(np.arange(64)))
_Q64[40] *= 200.0
TABLES = {"T20_K4": (20, 4, Q4, 0.01), "T2000_K64": (2000, 64, list(_Q64), 0.01)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def close(a, b):
    """tests/test_gpu_loss_options.py's loss tolerance, element by element."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) < 1e-6 * np.abs(b) + 1e-7))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _table_of(smp):
    return [int(v) for v in smp.c.cpu().tolist()], smp.iw.cpu().numpy()


# ---- 1. the draw kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(TABLES))
def test_draw_kernel_is_bitwise_the_reference(dev, case):
    from view_fusion_amd import ops
    T, K, q, eps = TABLES[case]
    B, seed = 1000, 0x1234_5678_9ABC_DEF1
    assert B > 64 and B % 64 != 0
    smp = ops.LevelSampler("fixed", T, dev, bins=K, probs=q, uniform_mix=eps)
    c, iw = _table_of(smp)
    c_ref, _ = lsr.table(q, T, K, eps)
    assert max(abs(a - b) for a, b in zip(c, c_ref)) <= 1 and np.array_equal(bits(iw), bits(lsr.iw_of(c, T, K)))
    gam = torch.linspace(0.999, 0.001, T, device=dev)
    ids = np.concatenate([np.arange(B - 3), [2 ** 40 + 7, 2 ** 62, -1]]).astype(np.int64)
    # seeded: word 0 of the training-scalars call -> t through the table; word 1 -> u
    t, level, u, w = ops.draw_level(smp, gam, seed=seed, ids=torch.from_numpy(ids).to(dev), want_u=True)
    words = rng_ref.words(seed, ids, rng_ref.KIND_SCALARS, 0, 1)[:, 0]
    t_ref, k_ref = lsr.draw(words[:, 0], c, T, K)
    _, u_ref = rng_ref.train_scalars(seed, ids, T)
    assert t.dtype == torch.int64 and np.array_equal(t.cpu().numpy(), t_ref)
    assert np.array_equal(bits(u.cpu().numpy()), bits(u_ref)) and np.array_equal(bits(w.cpu().numpy()), bits(iw[k_ref]))
    g64 = gam.double().cpu().numpy()
    want = (g64[t_ref] - g64[t_ref - 1]) * u_ref.astype(np.float64) + g64[t_ref - 1]
    assert np.abs(level.double().cpu().numpy() - want).max() <= 3 * 2.0 ** -24      # as tests/test_gpu_rng.py
    assert torch.equal(level, ops.gather_level(gam, t, u))
    differs = int((t_ref != lsr.uniform_draw(words[:, 0], T)).sum())
    print(f"{case}: {differs} of {B} draws differ from the uniform map; bins hit {len(set(k_ref.tolist()))} of {K}")
    assert differs > B // 4
    # words: the unseeded path, with every cut point's two sides among them
    rng = np.random.default_rng(3)
    edges = [0, (1 << 32) - 1] + [c[k] - 1 for k in range(1, K + 1)] + [c[k] for k in range(K)]
    x = np.concatenate([rng.integers(0, 1 << 32, B - len(edges), dtype=np.uint64), np.array(edges, dtype=np.uint64)])
    t2, level2, u2, w2 = ops.draw_level(smp, gam, words=torch.from_numpy(x.astype(np.int64)).to(dev))
    t2_ref, k2_ref = lsr.draw(x, c, T, K)
    assert level2 is None and u2 is None
    assert np.array_equal(t2.cpu().numpy(), t2_ref) and np.array_equal(bits(w2.cpu().numpy()), bits(iw[k2_ref]))
    assert t2_ref.min() == 1 and t2_ref.max() == T - 1
    with pytest.raises(ValueError):
        ops.draw_level(smp, gam)                                             # neither seed nor words
    with pytest.raises(ValueError):
        ops.draw_level(smp, gam[:-1], seed=1, ids=torch.zeros(1, dtype=torch.int64, device=dev))


# ---- 2. statistics and table -------------------------------------------------------------------------------------------
def test_statistics_kernel_updates_the_bins_and_rebuilds_the_table(dev):
    from view_fusion_amd import ops
    B, K, T, beta, eps = 70, 100, 401, 0.75, 0.01
    smp = ops.LevelSampler("loss_aware", T, dev, bins=K, ema=beta, warmup=1, uniform_mix=eps)
    lo = lsr.lo(T, K)
    g = torch.Generator().manual_seed(21)
    # call 1: bins 0..64 once, bins 0..4 a second time; call 2: bins 30..99, the sample of bin 30 with a NaN loss
    calls = [list(range(65)) + list(range(5)), list(range(30, 100))]
    m64, seen64 = np.zeros(K), np.zeros(K, dtype=np.int64)
    c0, iw0 = _table_of(smp)
    for call, bins_ in enumerate(calls):
        assert len(bins_) == B
        t = np.array([lo[k] + (k + call) % (lo[k + 1] - lo[k]) for k in bins_], dtype=np.int64)
        assert np.array_equal(lsr.bin_of(t, T, K), bins_)
        s = (0.2 + torch.rand(B, generator=g) * 3).numpy()
        w = (0.3 + torch.rand(B, generator=g) * 1.2).numpy()
        if call == 1:
            s[0] = np.nan
        m_prev = smp.m.cpu().numpy().astype(np.float64)
        ops.level_stats(smp, torch.from_numpy(s).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(t).to(dev))
        m64, seen64 = lsr.stats_update(m64, seen64, s, w, t, T, K, beta)
        m, seen = smp.m.cpu().numpy(), smp.seen.cpu().numpy()
        assert np.array_equal(seen, seen64)
        # fp32: (w s)^2 and a sum of at most 2 terms, the division, the EMA's subtract / multiply / add -- well inside
        # the B + 8 roundings per update the bound allows for; two updates: 2 (B + 8) 2^-24 = 9.3e-6 <= 1e-5
        e = float(np.abs(m - m64).max() / np.abs(m64).max())
        e_bin = float((np.abs(m - m64)[m64 > 0] / m64[m64 > 0]).max())
        print(f"call {call + 1}: seen {seen.sum()} samples in {int((seen > 0).sum())} bins  m vs float64: {e:.2e} of the "
              f"largest, {e_bin:.2e} per bin  ready {int(smp.ready)}")
        assert e_bin <= 1e-5
        if call == 0:                                # bins 65..99 are empty: not ready, the table is left alone
            assert int(smp.ready) == 0 and _table_of(smp)[0] == c0 and np.array_equal(_table_of(smp)[1], iw0)
            assert seen[:5].tolist() == [2] * 5 and seen[65:].sum() == 0 and (m[65:] == 0).all()
        else:
            assert seen[30] == 1 and m[30] == np.float32(m_prev[30])       # the NaN sample: skipped, bin 30 untouched
            assert seen[31:65].tolist() == [2] * 34                         # (the EMA branch ran)
    assert int(smp.ready) == 1
    c, iw = _table_of(smp)
    m_dev = smp.m.cpu().numpy()
    c_ref, _ = lsr.table(lsr.masses(m_dev, T, K), T, K, eps)             # from the device's own m
    d = max(abs(a - b) for a, b in zip(c, c_ref))
    print(f"table: max |c - c_ref(device m)| = {d} counts; p_k {min(np.diff(c)) / 2 ** 32:.3e} .. {max(np.diff(c)) / 2 ** 32:.3e}")
    assert d <= 1 and c[0] == 0 and c[K] == 1 << 32
    assert np.array_equal(bits(iw), bits(lsr.iw_of(c, T, K)))             # bitwise the formula on the device's own c
    p, seen_t, ready = smp.proposal()
    assert bool(ready) and abs(float(p.sum()) - 1.0) < 1e-12 and torch.equal(seen_t, smp.seen)
    with pytest.raises(ValueError):
        ops.level_stats(ops.LevelSampler("fixed", T, dev, bins=K, probs=[1.0] * K), smp.m[:B], None, smp.c[:B])


# ---- 3. warm-up ----------------------------------------------------------------------------------------------------------
def _model(dev, sched=SCHED):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": sched}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


def _batch(dev, B, vc, s=0):
    from view_fusion_amd import train
    return dict(train.synthetic_batch(B, 3, 16, dev, seed=40 + s), view_count=torch.tensor(vc))


def _grads(vf):
    return [p.grad.detach().cpu() for p in vf.parameters()]


def _on_loss_path(vf, dev, K=4):
    """A model WITHOUT a sampler on the compose_loss kernels: an attached histogram does that (train.Trainer(loss_bins=))."""
    vf.loss_hist = (torch.zeros(K, device=dev), torch.zeros(K, device=dev, dtype=torch.int32))
    return vf


def test_warmup_is_the_uniform_path_bit_for_bit(dev):
    from view_fusion_amd import ops
    B, vc, seed = 3, [1, 3, 2], 11
    ids = torch.arange(B, dtype=torch.int64, device=dev) + 5
    vf = _model(dev)
    vf.set_level_sampler("loss_aware", bins=4, warmup=1000)
    t0, level0, u0 = ops.draw_train(seed, ids, vf.gammas, want_u=True)
    t, level, u, iw = ops.draw_level(vf.level_sampler, vf.gammas, seed=seed, ids=ids, want_u=True)
    assert torch.equal(t, t0) and torch.equal(level, level0) and torch.equal(u, u0) and iw.tolist() == [1.0] * B
    batch = _batch(dev, B, vc)
    kw = dict(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"], seed=seed,
              sample_ids=ids)
    loss = vf(**kw)
    loss.backward()
    assert torch.equal(vf.last_t, t0) and vf.last_importance_weight.tolist() == [1.0] * B
    assert int(vf.level_sampler.seen.sum()) == B and int(vf.level_sampler.ready) == 0     # (the statistics did run)
    ref = _on_loss_path(_model(dev), dev)
    loss_r = ref(**kw)
    loss_r.backward()
    assert ref.last_t is None and ref.last_importance_weight is None
    assert torch.equal(loss.detach(), loss_r.detach()) and torch.equal(vf.last_sample_loss, ref.last_sample_loss)
    assert all(torch.equal(a, b) for a, b in zip(_grads(vf), _grads(ref)))
    # eval mode: the draw and the weight, but no update
    vf.eval()
    vf(**kw)
    assert int(vf.level_sampler.seen.sum()) == B
    # an injected t bypasses the sampler entirely
    vf.train()
    vf(**kw, t=t0)
    assert vf.last_t is None and vf.last_importance_weight is None and int(vf.level_sampler.seen.sum()) == B


def test_unseeded_path_draws_one_word_where_randint_draws_t(dev):
    """Without seed= the word comes from torch's device generator, one randint(0, 2^32) where t is drawn today, then u
    and the noise as before: replaying the generator gives the words, and the restatement gives t and the weight."""
    B, vc, T, K = 3, [1, 3, 2], 20, 4
    batch = _batch(dev, B, vc)
    kw = dict(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"])
    vf = _model(dev)
    vf.set_level_sampler("fixed", bins=K, probs=Q4)
    c, iw = _table_of(vf.level_sampler)
    torch.manual_seed(123)
    loss = vf(**kw)
    torch.manual_seed(123)
    words = torch.randint(0, 2 ** 32, (B,), device=dev)
    u = torch.rand((B, 1), device=dev)
    noise = torch.randn_like(batch["y_0"])
    t_ref, k_ref = lsr.draw(words.cpu().numpy().astype(np.uint64), c, T, K)
    assert np.array_equal(vf.last_t.cpu().numpy(), t_ref)
    assert np.array_equal(bits(vf.last_importance_weight.cpu().numpy()), bits(iw[k_ref]))
    # the same step with everything injected and no sampler: the same per-sample losses, and the loss is their weighted mean
    ref = _on_loss_path(_model(dev), dev)
    ref(**kw, t=vf.last_t, u=u, noise=noise)
    assert torch.equal(vf.last_sample_loss, ref.last_sample_loss) and torch.equal(vf.last_level, ref.last_level)
    assert close(float(loss.detach()), float((iw[k_ref].astype(np.float64) * vf.last_sample_loss.cpu().numpy()).mean()))


# ---- 4. compose_loss(sample_scale=) --------------------------------------------------------------------------------------
SHAPES = {"8x8": ((8, 8), (1, 3, 2)), "12x20": ((12, 20), (1, 3, 2))}
LEVEL3 = np.array([0.95, 0.4, 0.05], dtype=np.float32)
SCALE3 = np.array([0.3127, 94.01, 1.7], dtype=np.float32)                # the range of T20_K4's importance weights
WEIGHT_CASES = [(None, 0.0, 0.0), ("min_snr", 5.0, 0.0), ("p2", 1.0, 1.0)]
DELTA = 0.7
_INPUTS = {}


def _inputs(shape, weighting):
    """tests/test_gpu_loss_options.py's recipe: float64 |noise_hat - target| >= 1e-2 everywhere (L1's kink)."""
    key = (shape, weighting)
    if key not in _INPUTS:
        (H, W), vc = SHAPES[shape]
        g = torch.Generator().manual_seed(3)
        out = (torch.randn(sum(vc), 6, H, W, generator=g) * 2).numpy()
        nh, _ = loss_ref.compose(out, vc, weighting)
        mag = 0.01 + torch.randn(len(vc), 3, H, W, generator=g).abs().double().numpy()
        sign = np.where(torch.rand(len(vc), 3, H, W, generator=g).numpy() < 0.5, -1.0, 1.0)
        _INPUTS[key] = (out, (nh - sign * mag).astype(np.float32), vc)
    return _INPUTS[key]


@pytest.mark.parametrize("weighting", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_scaled_compose_loss_against_float64(dev, shape, weighting):
    from view_fusion_amd import ops
    out, target, vc = _inputs(shape, weighting)
    off, _, _ = ops.view_offsets(list(vc), dev)
    failures = []
    for penalty in loss_ref.PENALTIES:
        for kind, a, b in WEIGHT_CASES:
            ref = lsr.scaled_loss(out, target, vc, weighting, LEVEL3, SCALE3, penalty, DELTA, kind, a, b, gloss=1.7)
            og = torch.from_numpy(out).to(dev).requires_grad_(True)
            loss, sl, w = ops.compose_loss(og, torch.from_numpy(target).to(dev), off, len(vc), weighting,
                                           torch.from_numpy(LEVEL3).to(dev), penalty, DELTA, kind, a, b,
                                           sample_scale=torch.from_numpy(SCALE3).to(dev), want_weight=True)
            (loss * 1.7).backward()
            loss = loss.detach()
            e_loss = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
            e_sl = float((np.abs(sl.cpu().numpy() - ref["sample_loss"]) / np.abs(ref["sample_loss"])).max())
            e_d = rel(og.grad.cpu().numpy(), ref["dout"])
            print(f"{shape} softmax={weighting} {penalty:5s} {str(kind):7s}: loss {float(loss):.9g} (f64 {ref['loss']:.12g}) "
                  f"rel {e_loss:.2e}  sample_loss rel {e_sl:.2e}  dout rel {e_d:.2e}")
            if not (close(float(loss), ref["loss"]) and close(sl.cpu().numpy(), ref["sample_loss"]) and e_d < 1e-5):
                failures.append((penalty, kind, e_loss, e_sl, e_d))
            # the third output is the noise-level weight ALONE, bit for bit what the unscaled call uses
            _, _, w0 = ops.compose_loss(og.detach(), torch.from_numpy(target).to(dev), off, len(vc), weighting,
                                        torch.from_numpy(LEVEL3).to(dev), penalty, DELTA, kind, a, b, want_weight=True)
            assert torch.equal(w, w0)
    assert not failures, failures


@pytest.mark.parametrize("shape", list(SHAPES))
def test_scaled_entry_without_a_scale_is_the_plain_entry(dev, shape):
    """vf_compose_loss_fwd_scaled(scale = NULL) against vf_compose_loss_fwd on the same buffers: every output bit."""
    from view_fusion_amd import ops
    from view_fusion_amd.ops.core import _call, _ptr, _stream
    out, target, vc = _inputs(shape, True)
    B, (H, W) = len(vc), SHAPES[shape][0]
    off, _, _ = ops.view_offsets(list(vc), dev)
    o, tg, lv = torch.from_numpy(out).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(LEVEL3).to(dev)
    got = []
    for name in ("vf_compose_loss_fwd", "vf_compose_loss_fwd_scaled"):
        nh = torch.zeros(B, 3, H, W, device=dev)
        buf = torch.zeros(B * 66 + 1, device=dev)
        hist = (torch.ones(5, device=dev), torch.ones(5, device=dev, dtype=torch.int32))
        sl, sw, loss = buf[B * 64:B * 65], buf[B * 65:B * 66], buf[B * 66:]
        scale = (None,) if name.endswith("scaled") else ()
        _call(name, _ptr(o), ctypes.c_void_p(off.data_ptr()), _ptr(tg), _ptr(lv), *scale, _ptr(nh), _ptr(buf), _ptr(sl),
              _ptr(sw), _ptr(loss), _ptr(hist[0]), ctypes.c_void_p(hist[1].data_ptr()), B, 6, H * W, 1, 2, DELTA, 1, 5.0,
              0.0, 5, _stream())
        got.append((nh, buf, hist[0], hist[1]))
    assert all(torch.equal(a, b) for a, b in zip(*got)) and float(got[0][1][-1]) > 0


# ---- 5. / 6. model level ---------------------------------------------------------------------------------------------------
SCHED21 = dict(SCHED, num_timesteps=21)


def test_uniform_fixed_table_is_exactly_the_unsampled_step(dev):
    """T = 21, K = 4, uniform probs: every width is 2^30 and every importance weight 1.0, so the step is, bit for bit, the
    sampler-free step on the drawn t (both on the compose_loss kernels)."""
    from view_fusion_amd import ops
    B, vc, seed = 3, [1, 3, 2], 17
    ids = torch.arange(B, dtype=torch.int64, device=dev) + 9
    batch = _batch(dev, B, vc)
    kw = dict(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"])
    vf = _model(dev, SCHED21)
    vf.set_level_sampler("fixed", bins=4, probs=[0.25] * 4)
    c, iw = _table_of(vf.level_sampler)
    assert c == [k << 30 for k in range(5)] and iw.tolist() == [1.0] * 4
    loss = vf(**kw, seed=seed, sample_ids=ids)
    loss.backward()
    words = rng_ref.words(seed, ids.cpu().numpy(), rng_ref.KIND_SCALARS, 0, 1)[:, 0, 0]
    assert np.array_equal(vf.last_t.cpu().numpy(), lsr.draw(words, c, 21, 4)[0])
    assert vf.last_importance_weight.tolist() == [1.0] * B
    _, _, u = ops.draw_train(seed, ids, vf.gammas, want_u=True)
    noise = ops.randn_ids(seed, ids, ops.diffusion.RNG_TRAIN_NOISE, 0, (3, 16, 16))
    ref = _on_loss_path(_model(dev, SCHED21), dev)
    loss_r = ref(**kw, t=vf.last_t, u=u.reshape(B, 1), noise=noise)
    loss_r.backward()
    assert torch.equal(loss.detach(), loss_r.detach())
    assert all(torch.equal(a, b) for a, b in zip(_grads(vf), _grads(ref)))


def _seed_with_distinct_bins(T, K, c, ids, want):
    """The first seed whose draws from table c put the samples `ids` into `want` distinct bins (numpy, on the CPU)."""
    for seed in range(1, 500):
        x = rng_ref.words(seed, ids, rng_ref.KIND_SCALARS, 0, 1)[:, 0, 0]
        if len(set(lsr.draw(x, c, T, K)[1].tolist())) == want:
            return seed
    raise AssertionError("no seed found")


def test_skewed_batch_gradient_is_the_importance_weighted_sum_of_its_samples(dev):
    """B = 3, T20_K4's skewed table, min-SNR weighting on top: the parameter gradient equals
    sum_b iw_b w_b grad(loss_b) / B of three B = 1 default-path runs with the same draws injected, within 4 x the distance
    of the undivided DEFAULT batch from its own singles -- the rule and the measure of tests/test_gpu_loss_options.py."""
    B, vc, T, K = 3, [1, 3, 2], 20, 4
    ids_np = np.arange(B, dtype=np.int64) + B
    c_ref, _ = lsr.table(Q4, T, K, 0.01)
    seed = _seed_with_distinct_bins(T, K, c_ref, ids_np, 3)
    ids = torch.from_numpy(ids_np).to(dev)
    batch = _batch(dev, B, vc)
    kw = lambda sl: dict(y_cond=batch["y_cond"][sl], view_count=batch["view_count"][sl], angle=batch["angle"][sl],
                         y_0=batch["y_0"][sl], seed=seed, sample_ids=ids[sl])
    vf = _model(dev)
    vf.set_loss(weighting="min_snr", snr_gamma=1.0)
    vf.set_level_sampler("fixed", bins=K, probs=Q4)
    loss = vf(**kw(slice(0, B)))
    loss.backward()
    g_s = [g.numpy().astype(np.float64) for g in _grads(vf)]
    t, iw = vf.last_t.clone(), vf.last_importance_weight.cpu().numpy().astype(np.float64)
    c, iw_tab = _table_of(vf.level_sampler)
    x = rng_ref.words(seed, ids_np, rng_ref.KIND_SCALARS, 0, 1)[:, 0, 0]
    t_ref, k_ref = lsr.draw(x, c, T, K)
    assert np.array_equal(t.cpu().numpy(), t_ref) and len(set(k_ref.tolist())) == 3      # the condition the seed was picked for
    assert np.array_equal(iw, iw_tab[k_ref].astype(np.float64)) and iw.max() / iw.min() > 3
    w = loss_ref.weights(vf.last_level.cpu().numpy(), "min_snr", 1.0)
    assert close(float(loss.detach()), float((iw * w * vf.last_sample_loss.cpu().numpy()).mean()))
    singles = []
    for b in range(B):                                                  # default path, B = 1, the same draws
        one = _model(dev)
        one(**kw(slice(b, b + 1)), t=t[b:b + 1]).backward()
        singles.append([g.numpy().astype(np.float64) for g in _grads(one)])
    und = _model(dev)
    und(**kw(slice(0, B)), t=t).backward()                              # default path, undivided
    g_def = [g.numpy().astype(np.float64) for g in _grads(und)]

    def dist(got, wts):
        diff = scale = 0.0
        for i, g in enumerate(got):
            want = sum(wts[b] * singles[b][i] for b in range(B)) / B
            diff, scale = max(diff, float(np.abs(g - want).max())), max(scale, float(np.abs(want).max()))
        return diff / scale

    e1, es = dist(g_def, np.ones(B)), dist(g_s, iw * w)
    print(f"seed {seed}  t {t_ref}  iw {iw}  w {w}  default batch vs its singles {e1:.3e}  sampled batch vs weighted singles "
          f"{es:.3e}  bound {4 * e1:.3e}")
    assert e1 > 0 and es <= 4.0 * e1, (es, e1)
    assert dist(g_s, np.ones(B)) > 100 * e1                              # (the weights do change the gradient)


# ---- 7. Trainer ----------------------------------------------------------------------------------------------------------------
TB, TVC, TK, WARM = 8, [1, 3, 2, 2, 3, 1, 2, 2], 4, 3      # (both halves stack 8 views: one micro-batch geometry)
STEPS, FLIP = 6, 3                 # `ready` must flip at the end of step FLIP: step 3 is also the first captured step


def _seen_after(seed, steps, B=TB, T=20, K=TK):
    """Per-bin sample counts after each of `steps` uniform-draw steps of a Trainer(seed=) started at it = 0 (numpy)."""
    from view_fusion_amd import train
    seen, out = np.zeros(K, dtype=np.int64), []
    for it in range(1, steps + 1):
        ids = np.arange(B, dtype=np.int64) + train.step_sample_ids(it, B)
        x = rng_ref.words(seed, ids, rng_ref.KIND_SCALARS, 0, 1)[:, 0, 0]
        seen = seen + np.bincount(lsr.bin_of(lsr.uniform_draw(x, T), T, K), minlength=K)
        out.append(seen.copy())
    return out


def _pick_trainer_seed():
    for seed in range(1, 2000):
        s = _seen_after(seed, FLIP)
        if s[FLIP - 2].min() < WARM <= s[FLIP - 1].min():
            return seed
    raise AssertionError("no seed found")


def _trainer(dev, graph, seed, **kw):
    from view_fusion_amd import train
    vf = _model(dev)
    vf.set_loss(penalty="huber", delta=0.5, weighting="min_snr", snr_gamma=1.0)
    vf.set_level_sampler("loss_aware", bins=TK, warmup=WARM, ema=0.5)
    tr = train.Trainer(vf, lr_warmup=1, graph=graph, seed=seed, **kw)
    tr.it = 0
    return vf, tr


def _state(vf):
    s = vf.level_sampler
    return [s.m.clone(), s.seen.clone(), s.c.clone(), s.iw.clone(), s.ready.clone()]


def _run(dev, vf, tr, n, first=0):
    """-> per step: (loss, table before the step, t, iw, ready after)"""
    rows = []
    for s in range(first, first + n):
        c_before, ready_before = [int(v) for v in vf.level_sampler.c.cpu().tolist()], int(vf.level_sampler.ready)
        loss = tr.step(_batch(dev, TB, TVC, s)).clone()
        rows.append(dict(loss=loss, c=c_before, ready=ready_before, t=vf.last_t.cpu().numpy().copy(),
                         iw=vf.last_importance_weight.cpu().numpy().copy(), it=tr.it))
    return rows


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_trainer_replay_equals_eager_through_the_flip(dev, tmp_path):
    from view_fusion_amd import drivers, train
    seed = _pick_trainer_seed()
    (vf_e, tr_e), (vf_g, tr_g) = _trainer(dev, False, seed), _trainer(dev, True, seed)
    re, rg = _run(dev, vf_e, tr_e, STEPS), _run(dev, vf_g, tr_g, STEPS)
    assert tr_e.graph_steps == 0 and tr_g.graph_steps == STEPS - 2 and tr_g.mode == "graph"
    assert all(torch.equal(a["loss"], b["loss"]) for a, b in zip(re, rg))
    assert all(np.array_equal(a["t"], b["t"]) and np.array_equal(bits(a["iw"]), bits(b["iw"])) for a, b in zip(re, rg))
    assert _same(vf_e.parameters(), vf_g.parameters()) and _same(_state(vf_e), _state(vf_g))
    # the flip happened where the CPU said it would: steps 1..FLIP drew uniformly, the later ones from the table
    assert [r["ready"] for r in rg] == [0] * FLIP + [1] * (STEPS - FLIP)
    assert bool((vf_g.level_sampler.seen >= WARM).all())
    differs = 0
    for r in rg:
        ids = np.arange(TB, dtype=np.int64) + train.step_sample_ids(r["it"], TB)
        x = rng_ref.words(seed, ids, rng_ref.KIND_SCALARS, 0, 1)[:, 0, 0]
        uni = lsr.uniform_draw(x, 20)
        if not r["ready"]:
            assert np.array_equal(r["t"], uni) and r["iw"].tolist() == [1.0] * TB
            continue
        t_ref, k_ref = lsr.draw(x, r["c"], 20, TK)                       # the table as the step before left it
        assert np.array_equal(r["t"], t_ref)
        assert np.array_equal(bits(r["iw"]), bits(lsr.iw_of(r["c"], 20, TK)[k_ref]))
        differs += int((t_ref != uni).sum())
    p, seen, ready = tr_g.level_proposal()
    print(f"seed {seed}: after {STEPS} steps p = {p.cpu().numpy().round(4)}  seen {seen.cpu().numpy()}  "
          f"{differs} of {(STEPS - FLIP) * TB} post-flip draws differ from the uniform map")
    assert differs >= 1 and bool(ready) and abs(float(p.sum()) - 1) < 1e-12

    # a set_level_sampler() call after the capture: the graphs are dropped, the next steps run eagerly and are captured again
    for vf in (vf_e, vf_g):
        vf.set_level_sampler("loss_aware", bins=TK, warmup=WARM, ema=0.5)
    before = tr_g.graph_steps
    re, rg = _run(dev, vf_e, tr_e, 3, first=STEPS), _run(dev, vf_g, tr_g, 3, first=STEPS)
    assert tr_g.graph_steps == before + 1                                # two eager sightings, then one replay
    assert rg[0]["ready"] == 0                                           # (a new sampler: warming up again)
    assert all(torch.equal(a["loss"], b["loss"]) for a, b in zip(re, rg))
    assert _same(vf_e.parameters(), vf_g.parameters()) and _same(_state(vf_e), _state(vf_g))

    # checkpoint round trip: a fresh model + load_state_dict continues with the same bits for two steps
    path = str(tmp_path / "ckpt.pt")
    drivers.save_checkpoint(path, vf_e, tr_e.opt, it=tr_e.it, level_sampler=vf_e.level_sampler.state_dict())
    vf_n, tr_n = _trainer(dev, False, seed)
    extra = drivers.load_checkpoint(path, vf_n, tr_n.opt, device=dev)
    tr_n.it = extra["it"]
    assert _same(_state(vf_e), _state(vf_n)) and "level_sampler" in extra
    ra, rb = _run(dev, vf_e, tr_e, 2, first=STEPS + 3), _run(dev, vf_n, tr_n, 2, first=STEPS + 3)
    assert all(torch.equal(a["loss"], b["loss"]) and np.array_equal(a["t"], b["t"]) for a, b in zip(ra, rb))
    assert _same(vf_e.parameters(), vf_n.parameters()) and _same(_state(vf_e), _state(vf_n))
    assert list(vf_e.state_dict().keys()) == list(_model(dev).state_dict().keys())       # no buffer, no parameter


def test_trainer_accum_steps_replay_equals_eager(dev):
    seed = _pick_trainer_seed()
    (vf_e, tr_e), (vf_g, tr_g) = _trainer(dev, False, seed, accum_steps=2), _trainer(dev, True, seed, accum_steps=2)
    re, rg = _run(dev, vf_e, tr_e, 4), _run(dev, vf_g, tr_g, 4)
    assert tr_g.graph_steps == 2 * 4 - 2                                 # micro-batches: two eager sightings, then replays
    assert all(torch.equal(a["loss"], b["loss"]) for a, b in zip(re, rg))
    assert _same(vf_e.parameters(), vf_g.parameters()) and _same(_state(vf_e), _state(vf_g))
    assert int(vf_g.level_sampler.seen.sum()) == 4 * TB and vf_g.last_t.numel() == TB // 2   # every micro-batch updated


# ---- 8. the default is untouched ---------------------------------------------------------------------------------------------
def test_removed_sampler_leaves_the_default_step_alone(dev):
    from view_fusion_amd import ops
    B, vc = 3, [1, 3, 2]
    batch = _batch(dev, B, vc)
    runs = []
    for touch in (False, True):
        vf = _model(dev)
        if touch:
            vf.set_level_sampler("fixed", bins=4, probs=Q4)
            vf.set_level_sampler(None)
        ops.st.KERNEL_LOG = []
        try:
            loss = vf(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"],
                      seed=5, sample_ids=torch.arange(B, dtype=torch.int64, device=dev))
            loss.backward()
            names = [r[5] for r in ops.st.KERNEL_LOG]
        finally:
            ops.st.KERNEL_LOG = None
        runs.append((loss.detach().cpu(), _grads(vf), names))
        assert vf.last_t is None and vf.level_sampler is None and vf.last_sample_loss is None
    (la, ga, na), (lb, gb, nb) = runs
    assert torch.equal(la, lb) and all(torch.equal(x, y) for x, y in zip(ga, gb))
    assert na == nb and "vf_draw_train" in na and "vf_compose_fwd" in na and "vf_compose_mse_bwd" in na
    assert not [n for n in na if n in ("vf_draw_level", "vf_level_stats") or n.startswith("vf_compose_loss")]
    # and with a sampler the step is the same list with three names swapped, plus the statistics launch after the loss
    vf = _model(dev)
    vf.set_level_sampler("loss_aware", bins=4)
    ops.st.KERNEL_LOG = []
    try:
        vf(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"], seed=5,
           sample_ids=torch.arange(B, dtype=torch.int64, device=dev)).backward()
        names = [r[5] for r in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None
    swap = {"vf_draw_train": "vf_draw_level", "vf_compose_fwd": "vf_compose_loss_fwd_scaled",
            "vf_compose_mse_bwd": "vf_compose_loss_bwd"}
    want = [swap.get(n, n) for n in na]
    i = want.index("vf_compose_loss_fwd_scaled")
    assert names == want[:i + 1] + ["vf_level_stats"] + want[i + 1:]
