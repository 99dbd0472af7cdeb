"""The view store's data draws (csrc/rng.h kind 4, csrc/batch_plan.h) on the CPU: the numpy restatement's index algebra
against what the reference loader did (tests/golden/data_plan.npz), the library's host mirror against the restatement,
invariants, distribution and argument errors.  No GPU."""
import os

import numpy as np
import pytest
import torch

import data_ref
from test_rng_host import SEEDS

IDS = [0, 1, 2, 3, 1000, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 40] + list(range(7000, 7064))
DIST_SEED = 20250117                # test_distribution*: data_ref alone passes with it (checked before it was fixed)
KEYS = ("src", "target", "q01", "second", "view_count", "object")


@pytest.fixture(scope="module")
def data():
    import __graft_entry__ as ge
    ge.build()
    from view_fusion_amd import data
    return data


def host(data, seed, ids, train, lo, hi, N, objects=None):
    h = data.host_plan(seed, ids, "train" if train else "test", (lo, hi), N, objects)
    return {k: v.numpy().astype(np.int64) for k, v in h.items()}


def test_index_algebra_reproduces_the_reference_loader(golden_dir):
    g = np.load(os.path.join(golden_dir, "data_plan.npz"))
    second = (g["coin"] < 0.1) & g["train"]
    assert g["p"].shape == (400, 24) and int(second.sum()) >= 10 and not second[~g["train"]].any()
    r = data_ref.index_algebra(g["p"], second, g["q"])
    assert np.array_equal(r["target"], g["target"])
    assert np.array_equal(r["cond"], g["cond"])
    assert np.array_equal(r["rel_ref"], g["rel_ref"])
    assert np.array_equal(r["cond"], g["rel_cond"])
    for k in ("angle", "relative_angle"):
        assert r[k].dtype == g[k].dtype == np.float32 and np.array_equal(r[k].view(np.uint32), g[k].view(np.uint32)), k
    # the quirk that is kept: after a second shuffle relative_angle is NOT the angle between the views shown
    shown = (2 * np.pi / 24 * (r["src"][:, 1] - r["src"][:, 0])).astype(np.float32)
    assert (shown[second] != g["relative_angle"][second]).any()
    assert np.array_equal(shown[~second], g["relative_angle"][~second])


@pytest.mark.parametrize("N", [1, 5, 30000])
@pytest.mark.parametrize("lo,hi", [(1, 6), (7, 23)])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("seed", SEEDS)
def test_host_plan_is_bit_equal(data, seed, train, lo, hi, N):
    ids = np.array(IDS, dtype=np.int64)
    h, r = host(data, seed, ids, train, lo, hi, N), data_ref.plan(seed, ids, train, lo, hi, N)
    for k in KEYS:
        assert np.array_equal(h[k], np.asarray(r[k]).astype(np.int64)), k
    objects = (np.arange(ids.size) * 7) % N
    h, r = host(data, seed, ids, train, lo, hi, N, objects), data_ref.plan(seed, ids, train, lo, hi, N, objects)
    for k in KEYS:
        assert np.array_equal(h[k], np.asarray(r[k]).astype(np.int64)), k
    assert np.array_equal(h["object"], objects)


@pytest.mark.parametrize("train", [True, False])
def test_invariants(data, train):
    ids = np.arange(4096, dtype=np.int64) + 2 ** 33
    for lo, hi in ((1, 6), (7, 23), (3, 3)):
        h, r = host(data, 11, ids, train, lo, hi, 5), data_ref.plan(11, ids, train, lo, hi, 5)
        want = np.arange(24)
        for perm in (r["p"], r["q"], r["src"], h["src"]):
            assert (np.sort(perm, axis=1) == want).all()
        assert h["view_count"].min() >= lo and h["view_count"].max() <= hi
        assert h["object"].min() >= 0 and h["object"].max() < 5
        if train:
            assert 0 < h["second"].sum() < ids.size
            taken = h["second"].astype(bool)
            assert (h["src"][~taken, 0] == h["target"][~taken]).all()
        else:
            assert not h["second"].any() and not r["second"].any()
            assert (h["src"][:, 0] == h["target"]).all()


def _chi2(counts):
    e = counts.sum() / counts.size
    return float(((counts - e) ** 2 / e).sum())


def _distribution_checks(plan):
    """plan(ids) -> dict with target, second, view_count (1..6).  The input is fixed; the chi-square bounds are the
    0.99999 quantiles (23 dof: 64.0; 5 dof: 30.9), about the one-sided tail of five standard errors."""
    n = 24 * 4096
    p = plan(np.arange(n, dtype=np.int64))
    target, second, vc = (np.asarray(p[k]).astype(np.int64) for k in ("target", "second", "view_count"))
    c_t, c_v = np.bincount(target, minlength=24), np.bincount(vc - 1, minlength=6)
    frac, sigma = second.mean(), np.sqrt(0.1 * 0.9 / n)
    print(f"chi2 target {_chi2(c_t):.1f} (23 dof)  view_count {_chi2(c_v):.1f} (5 dof)  second {frac:.5f} "
          f"({(frac - 0.1) / sigma:+.2f} sigma)")
    assert c_t.size == 24 and c_v.size == 6
    assert _chi2(c_t) <= 64.0
    assert _chi2(c_v) <= 30.9
    assert abs(frac - 0.1) <= 5 * sigma


def test_distribution_of_the_restatement():
    _distribution_checks(lambda ids: data_ref.plan(DIST_SEED, ids, True, 1, 6, 5))


def test_distribution(data):
    _distribution_checks(lambda ids: host(data, DIST_SEED, ids, True, 1, 6, 5))


def test_argument_errors(data):
    ok = torch.zeros(2, 24, 3, 4, 4, dtype=torch.uint8)
    for bad in (ok.float(), ok[:, :23], torch.zeros(2, 24, 3, 3, 2, dtype=torch.uint8), ok[:, :, :2], ok[0], ok[:0]):
        with pytest.raises(ValueError):
            data.ViewStore(bad)
    for bad in (np.zeros((2, 24, 4, 4, 3), dtype=np.float32), np.zeros((2, 23, 4, 4, 3), dtype=np.uint8),
                np.zeros((2, 24, 3, 2, 3), dtype=np.uint8)):
        with pytest.raises(ValueError):
            data.ViewStore.from_hwc(bad, device="cpu")
    store = data.ViewStore(ok)                      # a host tensor is held, but nothing is assembled from it
    assert len(store) == 2 and (store.H, store.W) == (4, 4)
    for kw in (dict(objects=[0, 2]), dict(objects=[-1, 0]), dict(objects=[0]), dict(mode="val"), dict(view_range=(0, 3)),
               dict(view_range=(4, 24)), dict(view_range=(5, 4)), dict(max_views=24)):
        with pytest.raises(ValueError):
            store.batch(0, [0, 1], **kw)
    with pytest.raises(ValueError):
        store.batch(None, [0, 1])
    with pytest.raises(ValueError):
        list(store.eval_batches(2, None))
    with pytest.raises(ValueError):
        store.all_views([2])
    from view_fusion_amd._lib import VFHipError
    with pytest.raises(VFHipError):                 # valid arguments get as far as the launch: no CPU fallback
        store.batch(0, [0, 1])
    with pytest.raises(VFHipError):
        store.all_views([1])
    # the C entry points check on their own
    lib = data._lib.load()
    assert lib.vf_batch_host_plan(0, None, 1, 1, 0, 6, 5, *([None] * 7)) != 0
    assert lib.vf_batch_host_plan(0, None, 1, 1, 1, 24, 5, *([None] * 7)) != 0
    assert lib.vf_batch_host_plan(0, None, 1, 1, 1, 6, 0, *([None] * 7)) != 0
    assert lib.vf_batch_assemble(None, 5, 3, 2, 0, None, None, 1, 1, 0, 0, None, None, None, None, None) != 0


def test_trainer_draw_batch_needs_a_seed(data):
    from conftest import MICRO, SCHED_TRAIN
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.train import Trainer
    vf = ViewFusion(UNet(**MICRO), {"train": SCHED_TRAIN})
    store = data.ViewStore(torch.zeros(2, 24, 3, 16, 16, dtype=torch.uint8))
    with pytest.raises(ValueError):
        Trainer(vf, graph=False).draw_batch(store, 2)


def test_entry_points_are_declared_and_bound():
    import re
    from conftest import ROOT
    from view_fusion_amd import _lib
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    for name, n in (("vf_batch_assemble", 16), ("vf_batch_host_plan", 14)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]) == n, name
    spec = open(os.path.join(ROOT, "view_fusion_amd", "csrc", "rng.h")).read()
    assert "VF_RNG_DATA = 4" in spec and "kind 4" in spec
