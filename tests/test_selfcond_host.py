"""Self-conditioning on the host (the head of csrc/diffusion.hip holds the definition): the seeded coin (the library's host
mirror against the restatement of tests/selfcond_ref.py: word 3 of the call whose words 0..2 stay t, u and the conditioning
drop), the estimate's coefficients against the float64 formulas, the new entry points' declarations, and every refusal --
raised before anything touches the library.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import guidance_ref
import rng_ref
import selfcond_ref
from conftest import ROOT, SCHED_C1, TINY

NEW = ("vf_stack_views_sc", "vf_draw_self_cond", "vf_self_cond_estimate")
HOST = ("vf_self_cond_draw_host", "vf_self_cond_coeffs_host")
BIG = [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 33 + 9, 2 ** 63 - 1]
WIDE = dict(TINY, in_channel=9)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from view_fusion_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("p", [0.0, 0.25, 0.5, 1.0])
@pytest.mark.parametrize("seed", [0, 3, 0xDEADBEEFCAFEF00D, 2 ** 64 - 1])
def test_host_mirror_equals_the_restatement(lib, seed, p):
    from view_fusion_amd import ops
    assert ops.self_cond_threshold(p) == selfcond_ref.threshold(p)
    ids = np.concatenate([np.arange(5000), BIG]).astype(np.int64)
    got = ops.self_cond_draw_host(seed, torch.from_numpy(ids), p).numpy()
    want = selfcond_ref.coin(seed, ids, p)
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1} and np.array_equal(got.astype(bool), want)
    if p in (0.0, 1.0):
        assert got.all() == bool(p) and got.any() == bool(p)       # thr = 0: none; thr = 2^24: every 24-bit value is below it
    # the raw entry point, with a poisoned output buffer
    out = np.full(ids.size, 7, dtype=np.uint8)
    assert lib.vf_self_cond_draw_host(seed, ctypes.c_void_p(ids.ctypes.data), selfcond_ref.threshold(p),
                                      ctypes.c_void_p(out.ctypes.data), ids.size) == 0
    assert np.array_equal(out, got)
    assert lib.vf_self_cond_draw_host(seed, ctypes.c_void_p(ids.ctypes.data), 2 ** 24 + 1, ctypes.c_void_p(out.ctypes.data), 2) != 0


def test_thresholds():
    from view_fusion_amd import ops
    assert ops.self_cond_threshold(0.0) == 0 and ops.self_cond_threshold(1.0) == 2 ** 24
    assert ops.self_cond_threshold(0.5) == 2 ** 23 and ops.self_cond_threshold(2.0 ** -30) == 1
    for p in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.self_cond_threshold(p)


def test_rate_at_one_half(lib):
    from view_fusion_amd import ops
    n = 4096
    got = float(ops.self_cond_draw_host(2024, torch.arange(n), 0.5).float().mean())
    print(f"p = 0.5 over {n} ids: kept share {got:.4f} ({(got - 0.5) / (0.25 / n) ** 0.5:+.2f} sigma)")
    assert 4 * (0.25 / n) ** 0.5 == 0.03125 and abs(got - 0.5) <= 0.03125          # 4 standard deviations


def test_the_mask_of_an_id_does_not_depend_on_its_position(lib):
    from view_fusion_amd import ops
    ids = torch.tensor(list(range(40)) + BIG)
    base = ops.self_cond_draw_host(11, ids, 0.5)
    perm = torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(1))
    assert torch.equal(ops.self_cond_draw_host(11, ids[perm], 0.5), base[perm])
    for k in range(0, ids.numel(), 7):                       # one id alone, or in a batch of another size
        assert int(ops.self_cond_draw_host(11, ids[k:k + 1], 0.5)) == int(base[k])
        assert torch.equal(ops.self_cond_draw_host(11, ids[k:k + 3], 0.5), base[k:k + 3])
    assert 0 < int(base.sum()) < ids.numel()


def test_words_0_to_2_still_give_t_u_and_the_drop(lib):
    """The coin takes word 3 of the call; the library's other three readings of that call are rng_ref's, as before."""
    seed, T = 2024, 1000
    ids = np.concatenate([np.arange(2000), BIG]).astype(np.int64)
    t, u = np.empty(ids.size, dtype=np.int64), np.empty(ids.size, dtype=np.float32)
    assert lib.vf_rng_host_train_scalars(seed, ctypes.c_void_p(ids.ctypes.data), T, ctypes.c_void_p(t.ctypes.data),
                                         ctypes.c_void_p(u.ctypes.data), ids.size) == 0
    want_t, want_u = rng_ref.train_scalars(seed, ids, T)
    assert np.array_equal(t, want_t) and np.array_equal(u, want_u)
    drop = np.empty(ids.size, dtype=np.uint8)
    assert lib.vf_cond_drop_host(seed, ctypes.c_void_p(ids.ctypes.data), guidance_ref.drop_threshold(0.25),
                                 ctypes.c_void_p(drop.ctypes.data), ids.size) == 0
    assert np.array_equal(drop.astype(bool), guidance_ref.cond_drop(seed, ids, 0.25))
    # ... and the coin is its own word: not the drop's, and uncorrelated with t and u
    from view_fusion_amd import ops
    keep = ops.self_cond_draw_host(seed, torch.from_numpy(ids), 0.25).numpy()
    assert not np.array_equal(keep, drop)
    w = rng_ref.words(seed, ids, rng_ref.KIND_SCALARS, 0, 1)[:, 0]
    assert np.array_equal(keep.astype(bool), (w[:, 3] >> np.uint64(8)) < np.uint64(2 ** 22))
    k = keep.astype(np.float64)
    assert abs(np.corrcoef(k, t)[0, 1]) < 0.1 and abs(np.corrcoef(k, u)[0, 1]) < 0.1


@pytest.mark.parametrize("prediction", ["eps", "v", "x0"])
def test_coefficients_against_the_float64_formulas(lib, prediction):
    from view_fusion_amd import ops
    level = np.array([1e-4, 0.3, 0.9999], dtype=np.float32)
    a, b = (c.numpy() for c in ops.self_cond_coeffs_host(level, prediction))
    wa, wb = selfcond_ref.coeffs(level, prediction)
    for name, got, want in (("a", a, wa), ("b", b, wb)):
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want) / ulp
        print(f"{prediction} {name}: {got}  float64 {want}  error in fp32 ulps {err}")
        assert got.dtype == np.float32 and np.all(err <= 2.0)
    if prediction == "x0":
        assert a.tolist() == [0.0] * 3 and b.tolist() == [-1.0] * 3
    out = np.empty(3, dtype=np.float32)
    assert lib.vf_self_cond_coeffs_host(ctypes.c_void_p(level.ctypes.data), 3, ctypes.c_void_p(out.ctypes.data),
                                        ctypes.c_void_p(out.ctypes.data), 3) != 0


def test_new_entry_points_are_declared_bound_and_mapped():
    from view_fusion_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    listing = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW + HOST:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, f"{name} is not declared in include/vf_hip.h"
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == len(_lib.SIGNATURES[name]), name
        assert name in listing, f"{name} is not in INTEGRATION.md's ABI list"
    for name in NEW:
        assert ops.core._CALL_KIND[name] == "diffusion"
    # the stacking sibling is vf_stack_views_cfg plus one pointer; the existing two keep their signatures
    assert len(_lib.SIGNATURES["vf_stack_views"]) == 16 and len(_lib.SIGNATURES["vf_stack_views_cfg"]) == 18
    assert _lib.SIGNATURES["vf_stack_views_sc"] == _lib.SIGNATURES["vf_stack_views_cfg"][:7] + [ctypes.c_void_p] + \
        _lib.SIGNATURES["vf_stack_views_cfg"][7:]
    assert _lib.SIGNATURES["vf_draw_self_cond"] == _lib.SIGNATURES["vf_draw_cond_drop"]
    assert _lib.SIGNATURES["vf_self_cond_draw_host"] == _lib.SIGNATURES["vf_cond_drop_host"]
    for fn in ("draw_self_cond", "self_cond_estimate", "self_cond_threshold", "self_cond_draw_host"):
        assert callable(getattr(ops, fn))


def _cpu_model(hp=WIDE):
    from view_fusion_amd import UNet, ViewFusion
    vf = ViewFusion(UNet(**hp), {"train": SCHED_C1})
    vf.set_new_noise_schedule(device=torch.device("cpu"), phase="train")
    return vf


def test_every_refusal_comes_before_any_library_call(monkeypatch):
    from view_fusion_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was called")

    vf, narrow, teacher = _cpu_model(), _cpu_model(TINY), _cpu_model()
    n_state = len(vf.state_dict())
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)
    # the setting: a plain attribute and a key of the captured step
    assert vf.self_cond is None and vf.last_self_cond is None
    key = vf.loss_key()
    for p in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            vf.set_self_cond(p)
    assert vf.self_cond is None and vf.loss_key() == key
    vf.set_self_cond()
    assert vf.self_cond == 0.5 and vf.loss_key() != key and len(vf.state_dict()) == n_state
    k5 = vf.loss_key()
    vf.set_self_cond(0.25)
    assert vf.self_cond == 0.25 and vf.loss_key() not in (key, k5)
    vf.set_self_cond(None)
    assert vf.self_cond is None and vf.loss_key() == key
    # distillation on or with a self-conditioned model
    vf.set_self_cond(0.5)
    with pytest.raises(ValueError, match="self-conditioned"):
        vf.set_distill(teacher, steps=2)
    vf.set_self_cond(None)
    teacher.set_self_cond(0.5)
    with pytest.raises(ValueError, match="self-conditioned"):
        vf.set_distill(teacher, steps=2)
    teacher.set_self_cond(None)
    vf.set_distill(teacher, steps=2)
    with pytest.raises(ValueError, match="distillation"):
        vf.set_self_cond(0.5)
    vf.set_distill(None)
    # a level sampler together with self-conditioning, in either order
    vf.set_level_sampler("fixed", bins=3, probs=[1.0, 2.0, 1.0])
    with pytest.raises(ValueError, match="level sampler"):
        vf.set_self_cond(0.5)
    vf.set_level_sampler(None)
    vf.set_self_cond(0.5)
    with pytest.raises(ValueError, match="level sampler"):
        vf.set_level_sampler("fixed", bins=3, probs=[1.0, 2.0, 1.0])
    # a CPU model: every entry point that would run a self-conditioned pass
    B = 2
    args = (torch.rand(B, 2, 3, 16, 16), torch.tensor([2, 1]), torch.rand(B, 1))
    y = torch.rand(B, 3, 16, 16)
    for run in (lambda: vf(*args, y_0=y), lambda: vf(*args, y_0=y, seed=3), lambda: vf.self_cond_targets(*args, y),
                lambda: vf.generate(*args), lambda: vf(*args, generate=True, sample_steps=3),
                lambda: vf.p_sample(y, *args, torch.tensor([3, 3])),
                lambda: vf.p_mean_variance(y, *args, torch.tensor([3, 3]), True)):
        with pytest.raises(ValueError, match="GPU only"):
            run()
    vf.eval()
    with pytest.raises(ValueError, match="GPU only"):
        vf(*args, y_0=y)
    vf.train()
    # the in_channel mismatch names both numbers: a 6-channel stem under 3 conditioning channels, a 9-channel one under 6
    narrow.set_self_cond(0.5)
    for run in (lambda: narrow(*args, y_0=y), lambda: narrow.generate(*args), lambda: narrow.self_cond_targets(*args, y),
                lambda: narrow.p_sample(y, *args, torch.tensor([3, 3]))):
        with pytest.raises(ValueError, match=r"(?s)9.*in_channel = 6"):
            run()
    rel = (torch.rand(B, 2, 6, 16, 16),) + args[1:]
    with pytest.raises(ValueError, match=r"(?s)12.*in_channel = 9"):
        vf(*rel, y_0=y)
    # an injected estimate on a model that is not self-conditioned meets the same checks; a wrong shape is refused
    plain = _cpu_model(TINY)
    with pytest.raises(ValueError, match=r"in_channel = 6"):
        plain(*args, y_0=y, self_cond=torch.zeros_like(y))
    with pytest.raises(ValueError, match="set_self_cond"):
        plain.self_cond_targets(*args, y)
    # off again: the default forward gets as far as the first op, which refuses CPU tensors (no CPU fallback)
    vf.set_self_cond(None)
    with pytest.raises(_lib.VFHipError):
        _cpu_model(TINY)(*args, y_0=y)


def test_checkpoint_records_the_setting(tmp_path):
    from view_fusion_amd import drivers
    vf = _cpu_model()
    opt = torch.optim.Adam(vf.parameters(), lr=1e-4)
    vf.set_self_cond(0.25)
    path = os.path.join(tmp_path, "sc.pt")
    drivers.save_checkpoint(path, vf, opt, it=3, self_cond=vf.self_cond)
    other = _cpu_model()
    for p in (None, 0.5):
        other.set_self_cond(p)
        with pytest.raises(ValueError, match="self-conditioning"):
            drivers.load_checkpoint(path, other)
    other.set_self_cond(0.25)
    extra = drivers.load_checkpoint(path, other)
    assert extra["self_cond"] == 0.25 and extra["it"] == 3
    # a file without the entry loads as before, into either kind of model
    drivers.save_checkpoint(path, vf, opt, it=4)
    assert drivers.load_checkpoint(path, other)["it"] == 4
