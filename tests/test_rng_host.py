"""The seeded counter-based draws (csrc/rng.h) on the CPU: the library's host mirrors -- the very inline functions the
kernels run -- against the numpy restatement of tests/rng_ref.py.  No GPU."""
import ctypes

import numpy as np
import pytest

import rng_ref

SEEDS = [0, 1, 0x1234, 0xDEADBEEFCAFEF00D, 2 ** 64 - 1]
IDS = [0, 1, 2, 3, 1000, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 - 1, 2 ** 40]
DIST_SEED = 20240229                 # test_distribution: rng_ref alone passes with it (checked before it was fixed)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from view_fusion_amd import _lib
    return _lib.load()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def host_normal(lib, seed, ids, kind, step, n):
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    out = np.empty((ids.size, n), dtype=np.float32)
    assert lib.vf_rng_host_normal(seed, _p(ids), kind, step, _p(out), ids.size, n) == 0
    return out


def host_scalars(lib, seed, ids, T):
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    t, u = np.empty(ids.size, dtype=np.int64), np.empty(ids.size, dtype=np.float32)
    assert lib.vf_rng_host_train_scalars(seed, _p(ids), T, _p(t), _p(u), ids.size) == 0
    return t, u


def test_known_answers(lib):
    for ctr, key, want in rng_ref.KAT:
        assert rng_ref.philox_int(ctr, key) == want                      # the restatement itself
        assert tuple(int(w) for w in rng_ref.philox(*ctr, *key)) == want
        c, k, o = np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
        assert lib.vf_rng_host_philox(_p(c), _p(k), _p(o)) == 0
        assert tuple(int(x) for x in o) == want, [hex(int(x)) for x in o]


@pytest.mark.parametrize("T", [2, 10, 1000, 2000])
@pytest.mark.parametrize("seed", SEEDS)
def test_integers_and_uniforms_are_bit_equal(lib, seed, T):
    ids = np.array(IDS + list(range(5000, 5512)), dtype=np.int64)
    t, u = host_scalars(lib, seed, ids, T)
    tr, ur = rng_ref.train_scalars(seed, ids, T)
    assert np.array_equal(t, tr)
    assert u.dtype == ur.dtype == np.float32 and np.array_equal(u.view(np.uint32), ur.view(np.uint32))
    assert t.min() >= 1 and t.max() <= T - 1
    assert u.min() >= 0.0 and u.max() < 1.0
    if T == 2:
        assert (t == 1).all()
    if T >= 1000:
        assert len(set(t.tolist())) > 100                                # it does draw


@pytest.mark.parametrize("kind,step", [(1, 0), (2, 0), (3, 1), (3, 999), (3, 2 ** 28 - 1)])
@pytest.mark.parametrize("seed", SEEDS)
def test_normals_against_float64(lib, seed, kind, step):
    ids = np.array(IDS, dtype=np.int64)
    n = 3 * 16 * 16
    got = host_normal(lib, seed, ids, kind, step, n)
    r64, e, bound = rng_ref.bound(seed, ids, kind, step, n)
    err = float(np.abs(got.astype(np.float64) - r64).max())
    print(f"seed {seed:#x} kind {kind} step {step}: e {e:.3e}  bound {bound:.3e}  |host - fp64| {err:.3e}")
    assert err <= bound, (err, bound)
    assert np.abs(got).max() <= 6.77                                     # the stated cut of the tails


def test_kind_step_and_seed_separate_the_streams(lib):
    ids = np.arange(4, dtype=np.int64)
    base = host_normal(lib, 7, ids, 3, 5, 64)
    for other in (host_normal(lib, 8, ids, 3, 5, 64), host_normal(lib, 7, ids, 2, 5, 64),
                  host_normal(lib, 7, ids, 3, 6, 64), host_normal(lib, 7, ids + 4, 3, 5, 64),
                  host_normal(lib, 7 + 2 ** 32, ids, 3, 5, 64)):
        assert not np.array_equal(base, other)
    assert lib.vf_rng_host_normal(7, _p(ids), 4, 0, None, 4, 64) != 0   # kinds are 0..3
    assert lib.vf_rng_host_normal(7, _p(ids), 3, 2 ** 28, None, 4, 64) != 0
    assert lib.vf_rng_host_normal(7, _p(ids), 3, 0, None, 4, 6) != 0     # whole float4 blocks only


def _corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std()))


def _distribution_checks(draw):
    """draw(ids, step) -> (len(ids), n) normals of kind 3.  Five standard errors each; the input is fixed."""
    B, n = 64, 2 ** 14                                                    # 2^20 normals
    ids = np.arange(100, 100 + B + 1, dtype=np.int64)
    x = draw(ids, 7)
    a, nxt_id, nxt_step = x[:B], x[1:], draw(ids[:B], 8)
    N = a.size
    assert N >= 2 ** 20
    se = 1.0 / np.sqrt(N)
    stats = dict(mean=float(a.astype(np.float64).mean()), var=float(a.astype(np.float64).var()),
                 lag1=_corr(a[:, :-1], a[:, 1:]), ids=_corr(a, nxt_id), steps=_corr(a, nxt_step))
    print({k: f"{v:+.2e}" for k, v in stats.items()}, f"5 se = {5 * se:.2e}")
    assert abs(stats["mean"]) <= 5 * se
    assert abs(stats["var"] - 1.0) <= 5 * np.sqrt(2.0 / N)
    assert abs(stats["lag1"]) <= 5 * se and abs(stats["ids"]) <= 5 * se and abs(stats["steps"]) <= 5 * se


def test_distribution_of_the_restatement():
    _distribution_checks(lambda ids, step: rng_ref.normal(DIST_SEED, ids, 3, step, 2 ** 14, np.float32))


def test_distribution(lib):
    _distribution_checks(lambda ids, step: host_normal(lib, DIST_SEED, ids, 3, step, 2 ** 14))


def test_layout_independence(lib):
    whole = host_normal(lib, 5, [10, 11, 12, 13], 1, 0, 256)
    halves = np.concatenate([host_normal(lib, 5, [10, 11], 1, 0, 256), host_normal(lib, 5, [12, 13], 1, 0, 256)])
    assert np.array_equal(whole.view(np.uint32), halves.view(np.uint32))
    t, u = host_scalars(lib, 5, [10, 11, 12, 13], 1000)
    t2, u2 = host_scalars(lib, 5, [13, 10], 1000)
    assert t2.tolist() == [t[3], t[0]] and u2.tolist() == [u[3], u[0]]
    # a longer sample starts with the shorter one's draws: element e depends on its float4 index only
    assert np.array_equal(host_normal(lib, 5, [10], 1, 0, 512)[:, :256], whole[:1])


def test_trainer_id_arithmetic():
    """Same iteration, world 1 with batch 2B against world 2 with batch B per rank: one id set; no id twice in a run."""
    from view_fusion_amd.train import step_sample_ids
    B = 8
    seen = set()
    for it in range(5):
        one = {step_sample_ids(it, 2 * B) + b for b in range(2 * B)}
        two = {step_sample_ids(it, B, rank=r, world=2) + b for r in range(2) for b in range(B)}
        assert one == two and len(one) == 2 * B
        assert not (seen & one)
        seen |= one
    # an explicit global batch (ranks that hold less than their share of it) keeps iterations apart
    assert step_sample_ids(3, 4, rank=1, world=2, global_batch=16) == 3 * 16 + 4
    with pytest.raises(ValueError):
        step_sample_ids(0, 8, rank=1, world=2, global_batch=8)
