"""Loss-aware noise-level sampling on the CPU (csrc/level_sampler.h): the numpy restatement tests/level_sampler_ref.py
against the specification's own invariants (exact integer counting), the library's host mirrors of the table and the draw
against the restatement, the statistics rule on worked examples, set_level_sampler's argument checks, the Trainer's
refusals and the C ABI.  No GPU."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import level_sampler_ref as lsr
from conftest import ROOT, TINY

EPS = 0.01
# Strongly skewed masses: T = 20 with K = 4 (K does not divide T - 1 = 19: bins of 5, 5, 5, 4) and T = 2000 with K = 64.
# (T, K, masses, uniform_mix).  Within a bin the draw gives timestep j of n_k the words ceil((j+1) width_k / n_k) -
# ceil(j width_k / n_k): within ONE word of width_k / n_k.  So P(t) iw(t) differs from 1 / (T - 1) by at most the
# fraction n_k / width_k (+ 2^-24, the fp32 rounding of iw), and for a positive f the importance-weighted mean is within
# max_k n_k / width_k + 2^-24 of the uniform mean, relatively -- for ARBITRARY f that is attained (f = one timestep of
# the thinnest bin).  The 1e-6 the feature promises for arbitrary f therefore needs width_k / n_k >= ~1.1e6 in every bin,
# i.e. p_k >= n_k 2.5e-4: at T = 20 the default uniform_mix = 0.01 gives that (p_k >= 0.0021), at T = 2000 / K = 64
# (n_k = 31, 32) it needs p_k >= 0.0079, which uniform_mix = 0.51 provides while the masses still span e^9 and one bin holds
# most of the rest.  The third case keeps uniform_mix = 0.01 at T = 2000: the thinnest bins get ~21 000 words per timestep,
# and what holds there is the derived bound (~4.7e-5), not 1e-6.
_Q64 = np.exp(np.linspace(-6.0, 3.0, 64)) * (1.0 + 0.5 * np.sin(np.arange(64)))
_Q64[40] *= 200.0
CASES = {"T20_K4": (20, 4, [1.0, 50.0, 0.01, 8.0], EPS),
         "T2000_K64": (2000, 64, list(_Q64), 0.51),
         "T2000_K64_thin": (2000, 64, list(_Q64), EPS)}
ISSUE_BOUND = {"T20_K4": 1e-6, "T2000_K64": 1e-6, "T2000_K64_thin": None}
SCHED10 = dict(schedule="linear", num_timesteps=10, linear_start=1e-4, linear_end=0.09)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from view_fusion_amd import _lib
    return _lib.load()


def _host_table(q, T, K, eps=EPS):
    from view_fusion_amd import ops
    c, lo, iw = ops.level_table_host(q, T, K, eps)
    return [int(v) for v in c.tolist()], lo.tolist(), iw.numpy()


def test_bins_partition_the_timesteps():
    for T, K in ((20, 4), (2000, 64), (21, 4), (401, 100), (11, 10), (2, 1), (1025, 1024)):
        lo, n = lsr.lo(T, K), lsr.sizes(T, K)
        assert lo[0] == 1 and lo[K] == T and min(n) >= 1 and max(n) - min(n) <= 1 and sum(n) == T - 1
        t = np.arange(1, T)
        b = lsr.bin_of(t, T, K)
        for k in range(K):                                            # bin(t) == k exactly on [lo_k, lo_{k+1})
            assert np.array_equal(t[b == k], np.arange(lo[k], lo[k + 1])), (T, K, k)


@pytest.mark.parametrize("case", list(CASES))
def test_table_invariants_and_unbiasedness(case):
    T, K, q, eps = CASES[case]
    assert max(q) / min(q) > 1000
    c, iw = lsr.table(q, T, K, eps)
    n = lsr.sizes(T, K)
    width = [c[k + 1] - c[k] for k in range(K)]
    assert c[0] == 0 and c[K] == 1 << 32 and all(w >= nk for w, nk in zip(width, n))
    assert all(c[k] <= c[k + 1] for k in range(K))
    assert lsr.mean_iw_exact(c, T, K) == 1                            # rational arithmetic: exactly 1
    mean_iw = sum(Fraction(width[k]) * Fraction(float(iw[k])) for k in range(K)) / (1 << 32)
    print(f"{case}: widths {min(width)} .. {max(width)}  iw {iw.min():.4g} .. {iw.max():.4g}  "
          f"|mean iw - 1| {abs(float(mean_iw - 1)):.2e}")
    assert abs(float(mean_iw - 1)) <= 1e-6                            # only the fp32 rounding of iw
    # exact counting: every word lands on one timestep, every timestep keeps at least one word
    counts = lsr.word_counts(c, T, K)
    assert sorted(counts) == list(range(1, T)) and sum(counts.values()) == 1 << 32 and min(counts.values()) >= 1
    b = lsr.bin_of(np.arange(1, T), T, K)
    derived = max(Fraction(nk, w) for nk, w in zip(n, width)) + Fraction(1, 1 << 24)
    print(f"  derived bound max n_k / width_k + 2^-24 = {float(derived):.3e}  (p_k {min(width) / 2 ** 32:.4g} .. "
          f"{max(width) / 2 ** 32:.4g})")
    if ISSUE_BOUND[case] is not None:
        assert derived <= ISSUE_BOUND[case]
    for name, f in (("t^2", lambda t: Fraction(t * t)), ("1/t", lambda t: Fraction(1, t)),
                    ("zigzag", lambda t: Fraction((-1) ** t * (t % 7) + 8)),
                    ("one timestep of the thinnest bin", lambda t, tt=lsr.lo(T, K)[int(np.argmin(width))]: Fraction(int(t == tt)))):
        est = sum(Fraction(counts[t], 1 << 32) * Fraction(float(iw[b[t - 1]])) * f(t) for t in range(1, T))
        uni = sum(f(t) for t in range(1, T)) / (T - 1)
        err = abs(float((est - uni) / uni))
        print(f"  f = {name}: importance-weighted mean vs uniform mean, relative {err:.2e}")
        assert err <= float(derived), (name, err)
        if ISSUE_BOUND[case] is not None:
            assert err <= ISSUE_BOUND[case], (name, err)
    # (the proposal is really skewed: the unweighted mean is far off)
    raw = sum(Fraction(counts[t], 1 << 32) * t * t for t in range(1, T))
    assert abs(float(raw / (sum(Fraction(t * t) for t in range(1, T)) / (T - 1)) - 1)) > 0.05
    assert max(width) / min(width) > 30


@pytest.mark.parametrize("case", list(CASES))
def test_host_table_mirror_within_one_count(lib, case):
    """float64 in-order sums of at most 1024 terms: relative error ~1e-13, and 2^32 x 1e-13 << 1, so only a floor boundary
    can flip: at most 1 count per cut point.  lo is exact; iw is bitwise the formula on the mirror's own cut points."""
    T, K, q, eps = CASES[case]
    c_ref, _ = lsr.table(q, T, K, eps)
    c, lo, iw = _host_table(q, T, K, eps)
    d = max(abs(a - b) for a, b in zip(c, c_ref))
    print(f"{case}: max |c_host - c_ref| = {d} counts")
    assert d <= 1 and c[0] == 0 and c[K] == 1 << 32
    assert lo == lsr.lo(T, K)
    assert np.array_equal(iw.view(np.int32), lsr.iw_of(c, T, K).view(np.int32))


def test_host_table_mirror_uniform_case_is_exact(lib):
    c, lo, iw = _host_table([3.0] * 4, 21, 4)                          # T = 21, K = 4: every width 2^30, every iw 1
    assert c == [k << 30 for k in range(5)] and lo == [1, 6, 11, 16, 21] and iw.tolist() == [1.0] * 4


@pytest.mark.parametrize("case", list(CASES))
def test_host_draw_mirror_bitwise(lib, case):
    from view_fusion_amd import ops
    T, K, q, eps = CASES[case]
    c, iw = lsr.table(q, T, K, eps)
    rng = np.random.default_rng(5)
    edges = [0, (1 << 32) - 1] + [c[k] - 1 for k in range(1, K + 1)] + [c[k] for k in range(K)]
    x = np.concatenate([rng.integers(0, 1 << 32, 4096, dtype=np.uint64), np.array(edges, dtype=np.uint64)])
    t_ref, k_ref = lsr.draw(x, c, T, K)
    t, w = ops.level_draw_host(torch.from_numpy(x.astype(np.int64)), T, K, torch.tensor(c, dtype=torch.int64),
                               torch.from_numpy(iw))
    assert np.array_equal(t.numpy(), t_ref) and t_ref.min() == 1 and t_ref.max() == T - 1
    assert np.array_equal(w.numpy().view(np.int32), iw[k_ref].view(np.int32))
    assert np.array_equal(lsr.bin_of(t_ref, T, K), k_ref)              # the drawn t lies in the drawn bin
    # the draw agrees with the exact counts: a word below c_1 gives a timestep of bin 0, in rising order
    order = np.argsort(x, kind="stable")
    assert np.all(np.diff(t_ref[order]) >= 0)
    with pytest.raises(ValueError):                                     # not a table: c does not end at 2^32
        ops.level_draw_host(torch.zeros(1, dtype=torch.int64), T, K, torch.arange(K + 1), torch.from_numpy(iw))


def test_statistics_restatement():
    """First update, a later update (EMA), an empty bin, a skipped non-finite sample -- by hand."""
    T, K, beta = 21, 4, 0.75
    t = np.array([1, 5, 6, 20, 2, 16])                                 # bins 0, 0, 1, 3, 0, 3; bin 2 stays empty
    s = np.array([2.0, 4.0, 1.0, 3.0, np.nan, 0.5])
    w = np.array([1.0, 0.5, 2.0, 1.0, 1.0, 2.0])
    m, seen = lsr.stats_update(np.zeros(K), np.zeros(K, dtype=np.int64), s, w, t, T, K, beta)
    assert seen.tolist() == [2, 1, 0, 2]                               # the NaN sample is not counted
    assert m.tolist() == [(4.0 + 4.0) / 2, 4.0, 0.0, (9.0 + 1.0) / 2]
    assert not lsr.is_ready(m, seen, T, K, 1) and lsr.is_ready(m, np.maximum(seen, 1), T, K, 1)
    m2, seen2 = lsr.stats_update(m, seen, np.array([6.0, np.inf]), None, np.array([3, 11]), T, K, beta)
    assert seen2.tolist() == [3, 1, 0, 2]                              # Inf skipped: bin 2 still empty
    assert m2[0] == 4.0 + 0.25 * (36.0 - 4.0) and m2[1:].tolist() == m[1:].tolist()
    q = lsr.masses(m2, T, K)
    assert q.tolist() == [5 * np.sqrt(12.0), 5 * 2.0, 0.0, 5 * np.sqrt(5.0)]
    assert lsr.is_ready(m2, seen2 + 1, T, K, 1) and not lsr.is_ready(m2, seen2 + 1, T, K, 2)
    assert not lsr.is_ready(np.zeros(K), np.ones(K), T, K, 1)          # sum q == 0: never ready


def _cpu_model(T=10):
    from view_fusion_amd import UNet, ViewFusion
    vf = ViewFusion(UNet(**TINY), {"train": dict(SCHED10, num_timesteps=T)})
    vf.set_new_noise_schedule(device=torch.device("cpu"), phase="train")
    return vf


def test_set_level_sampler_validates_and_stores_no_state(lib):
    from view_fusion_amd import UNet, ViewFusion
    with pytest.raises(ValueError):                                     # no schedule yet: T is unknown
        ViewFusion(UNet(**TINY), {"train": SCHED10}).set_level_sampler("loss_aware")
    vf = _cpu_model(10)
    keys, key = list(vf.state_dict().keys()), vf.loss_key()
    bad = [dict(kind="importance"), dict(kind="loss_aware", bins=10), dict(kind="loss_aware", bins=0),
           dict(kind="loss_aware", bins=2.0), dict(kind="loss_aware", bins=3, uniform_mix=1e-9),
           dict(kind="loss_aware", bins=3, uniform_mix=1.5), dict(kind="loss_aware", bins=3, ema=1.0),
           dict(kind="loss_aware", bins=3, warmup=-1), dict(kind="loss_aware", bins=3, probs=[1, 1, 1]),
           dict(kind="fixed", bins=3), dict(kind="fixed", bins=3, probs=[1.0, 2.0]),
           dict(kind="fixed", bins=3, probs=[1.0, -2.0, 1.0]), dict(kind="fixed", bins=3, probs=[0.0, 0.0, 0.0]),
           dict(kind="fixed", bins=3, probs=[1.0, float("nan"), 1.0])]
    for kw in bad:
        with pytest.raises(ValueError):
            vf.set_level_sampler(**kw)
        assert vf._level_spec is None, kw                               # a refused call changes nothing
    # eps 2^32 >= 2 (T - 1) is the exact boundary
    from view_fusion_amd import ops
    lo_eps = lsr.min_uniform_mix(10)
    ops.check_level_sampler("loss_aware", 10, 3, None, 0.9, 10, lo_eps)
    with pytest.raises(ValueError):
        ops.check_level_sampler("loss_aware", 10, 3, None, 0.9, 10, lo_eps * (1 - 1e-12))
    vf.set_level_sampler("fixed", bins=9, probs=[1.0] * 9)              # K = T - 1 is allowed
    assert vf._level_spec["bins"] == 9 and vf.loss_key() != key
    assert vf.level_sampler is None                                     # a CPU model holds the settings only ...
    with pytest.raises(ValueError):                                     # ... and refuses to run with them
        vf(y_cond=torch.zeros(1, 1, 3, 16, 16), view_count=[1], angle=torch.zeros(1, 1), y_0=torch.zeros(1, 3, 16, 16))
    vf.set_level_sampler("loss_aware")
    assert vf._level_spec["bins"] == 9 and vf._level_spec["ema"] == 0.9 and vf._level_spec["warmup"] == 10
    vf.set_level_sampler(None)
    assert vf._level_spec is None and vf.level_sampler is None
    assert list(vf.state_dict().keys()) == keys and not [n for n, _ in vf.named_buffers() if "level" in n]


def test_trainer_refuses_a_sampler_on_the_cpu_and_across_ranks(lib):
    from view_fusion_amd import train
    vf = _cpu_model(10)
    vf.set_level_sampler("loss_aware", bins=3)
    with pytest.raises(ValueError, match="GPU"):
        train.Trainer(vf)                                               # a CPU model
    tr = train.Trainer(_cpu_model(10))
    tr.world = 2                                                        # (constructing world = 2 needs a process group)
    tr.module.set_level_sampler("loss_aware", bins=3)
    with pytest.raises(ValueError, match="single-process"):
        tr._check_level_sampler()
    with pytest.raises(ValueError):
        train.Trainer(_cpu_model(10)).level_proposal()


def test_abi_has_the_level_sampler_entries(lib):
    from view_fusion_amd import _lib
    from view_fusion_amd.ops import core
    header = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    for name, n in (("vf_compose_loss_fwd_scaled", 23), ("vf_draw_level", 15), ("vf_level_stats", 15),
                    ("vf_level_table_host", 7), ("vf_level_draw_host", 8)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/vf_hip.h"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name]) == n, name
        assert hasattr(lib, name)
    for name in ("vf_compose_loss_fwd_scaled", "vf_draw_level", "vf_level_stats"):
        assert core._CALL_KIND[name] == "diffusion"
    # the scaled entry is the plain one plus one pointer in fifth place; the plain one keeps its 22 arguments
    plain, scaled = _lib.SIGNATURES["vf_compose_loss_fwd"], _lib.SIGNATURES["vf_compose_loss_fwd_scaled"]
    assert len(plain) == 22 and scaled[:4] + scaled[5:] == plain and scaled[4] is _lib._P
    assert _lib.SIGNATURES["vf_level_stats"][8] is ctypes.c_double and _lib.SIGNATURES["vf_level_table_host"][3] is ctypes.c_double
    # the host mirrors refuse what the specification excludes
    q = np.ones(4)
    c, lo, iw = np.zeros(5, dtype=np.uint64), np.zeros(5, dtype=np.int32), np.zeros(4, dtype=np.float32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.vf_level_table_host(P(q), 21, 4, 0.01, P(c), P(lo), P(iw)) == 0
    assert lib.vf_level_table_host(P(q), 21, 4, 1e-9, P(c), P(lo), P(iw)) != 0      # eps too small
    assert lib.vf_level_table_host(P(q), 4, 4, 0.01, P(c), P(lo), P(iw)) != 0       # K > T - 1
    assert lib.vf_level_table_host(P(np.zeros(4)), 21, 4, 0.01, P(c), P(lo), P(iw)) != 0
