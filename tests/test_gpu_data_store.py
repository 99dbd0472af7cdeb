"""data.ViewStore on the GPU (csrc/batch.hip: vf_batch_assemble) against the numpy restatement tests/data_ref.py, bit for
bit (array_equal on the uint32 view): train / test mode, relative on / off, explicit objects, ids >= 2^32; row, batch and
order independence; out=; all_views; the NaN guard of the raw entry point; 64-bit store offsets on a store
whose last object lies beyond 2^32 bytes; Trainer.draw_batch against step() on the restatement's batch (loss bit for
bit, eager and replayed); eval_batches through drivers.evaluate at two batch sizes."""
import ctypes

import numpy as np
import pytest
import torch

import data_ref
from conftest import SCHED_C1, TINY

pytestmark = pytest.mark.gpu
SEED, N = 0, 5
IDS = list(range(64))
BIG = [2 ** 32, 2 ** 32 + 1, 2 ** 40, 2 ** 31, 2 ** 31 - 1, 7]
CHAIN_TOL = 1e-3                    # the same chain under another batching, max-abs of the samples


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bytes(shape, seed):
    """Random bytes; the first 256 of every view's 3 * H * W are a permutation of 0..255 when the view is that large."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=shape, dtype=np.uint8)
    flat = a.reshape(shape[0], shape[1], -1)
    if flat.shape[2] >= 256:
        for o in range(shape[0]):
            for v in range(shape[1]):
                flat[o, v, :256] = rng.permutation(256).astype(np.uint8)
    return flat.reshape(shape)


@pytest.fixture(scope="module", params=[(8, 12), (4, 4)], ids=["8x12", "4x4"])
def stores(request, dev):
    from view_fusion_amd import data
    H, W = request.param
    host = _bytes((N, 24, 3, H, W), 100 + H)
    if 3 * H * W >= 256:
        assert all(len(set(host[o, v].ravel().tolist())) == 256 for o in range(N) for v in range(24))
    return host, data.ViewStore(torch.from_numpy(host).to(dev))


def _u32(a):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(batch, host, pl, relative):
    y_0, y_cond, angle = data_ref.assemble(host, pl, relative)
    assert set(batch) == {"y_0", "y_cond", "angle", "view_count"}
    assert tuple(batch["y_cond"].shape) == y_cond.shape and tuple(batch["angle"].shape) == angle.shape == (len(y_0), 1)
    assert all(batch[k].dtype == torch.float32 and batch[k].is_cuda for k in ("y_0", "y_cond", "angle"))
    assert np.array_equal(_u32(batch["y_0"]), _u32(y_0))
    assert np.array_equal(_u32(batch["y_cond"]), _u32(y_cond))
    assert np.array_equal(_u32(batch["angle"]), _u32(angle))
    vc = batch["view_count"]
    assert not vc.is_cuda and vc.dtype == torch.int64 and np.array_equal(vc.numpy(), pl["view_count"])


def test_the_ids_exercise_every_branch():
    pl = data_ref.plan(SEED, IDS, True, 1, 6, N)
    taken = int(pl["second"].sum())
    print(f"second shuffle: {taken} of {len(IDS)}; view_count {sorted(set(pl['view_count'].tolist()))}; objects "
          f"{sorted(set(pl['object'].tolist()))}; {len(set(pl['target'].tolist()))} target views")
    assert taken >= 2 and len(IDS) - taken >= 2
    assert set(pl["view_count"].tolist()) == {1, 2, 3, 4, 5, 6} and set(pl["object"].tolist()) == set(range(N))


@pytest.mark.parametrize("relative", [False, True], ids=["plain", "relative"])
@pytest.mark.parametrize("mode", ["train", "test"])
def test_batch_is_bit_equal_to_the_restatement(stores, mode, relative):
    host, store = stores
    for ids, objects, rng in ((IDS, None, (1, 6)), (BIG, None, (1, 6)), (IDS[:9], [4, 0, 1, 2, 3, 4, 4, 0, 2], (7, 23))):
        pl = data_ref.plan(SEED, ids, mode == "train", rng[0], rng[1], N, objects)
        batch, plan = store.batch(SEED, ids, mode=mode, relative=relative, objects=objects,
                                  view_range=None if rng == (1, 6) else rng, return_plan=True)
        _check(batch, host, pl, relative)
        assert np.array_equal(plan["src"].numpy(), pl["src"]) and np.array_equal(plan["object"].numpy(), pl["object"])
    # another seed is another batch; a given view_count replaces the drawn one and nothing else
    pl = data_ref.plan(SEED + 1, IDS, mode == "train", 1, 6, N)
    other = store.batch(SEED + 1, torch.tensor(IDS), mode=mode, relative=relative, view_count=[2] * len(IDS))
    assert other["view_count"].tolist() == [2] * len(IDS)
    _check(dict(other, view_count=torch.from_numpy(pl["view_count"])), host, pl, relative)
    assert not np.array_equal(pl["target"], data_ref.plan(SEED, IDS, mode == "train", 1, 6, N)["target"])


def test_every_byte_converts_as_numpy_does(stores):
    host, store = stores
    want = (np.arange(256, dtype=np.uint8).astype(np.float32) / np.float32(255)).view(np.uint32)
    views = store.all_views(list(range(N)))
    assert np.array_equal(_u32(views), _u32(data_ref.pixels(host)))
    if host[0, 0].size >= 256:
        got = _u32(views)[0, 0].ravel()[np.argsort(host[0, 0].ravel()[:256], kind="stable")]
        assert np.array_equal(got, want)
    one = store.all_views(3)
    assert tuple(one.shape) == (1, 24, 3, store.H, store.W) and torch.equal(one[0], views[3])
    out = torch.empty_like(one)
    assert store.all_views([3], out=out) is out and torch.equal(out, one)


def test_rows_do_not_depend_on_batch_or_order(stores):
    _, store = stores
    a, b, c, x, y = 5, 2 ** 35 + 3, 40, 17, 63
    small = store.batch(SEED, [a, b, c], relative=True)
    large = store.batch(SEED, [c, x, a, y, b], relative=True)
    for k in ("y_0", "y_cond", "angle"):
        assert torch.equal(small[k], large[k][[2, 4, 0]]), k
    assert small["view_count"].tolist() == large["view_count"][[2, 4, 0]].tolist()


def test_out_writes_in_place(stores):
    _, store = stores
    fresh = store.batch(SEED, IDS[:6])
    out = {k: torch.full_like(v, float("nan")) for k, v in fresh.items() if k != "view_count"}
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    got = store.batch(SEED, IDS[:6], out=out)
    for k in out:
        assert got[k] is out[k] and got[k].data_ptr() == ptrs[k] and torch.equal(got[k], fresh[k]), k
    with pytest.raises(ValueError):
        store.batch(SEED, IDS[:6], out=dict(y_0=torch.empty(5, 3, store.H, store.W, device=store.device)))
    with pytest.raises(ValueError):
        store.batch(SEED, IDS[:6], out=dict(angle=torch.empty(6, 2, device=store.device)[:, :1]))


def test_an_object_outside_the_store_reads_nothing(stores, dev):
    """The raw entry point with device-side objects the Python layer would have refused: NaN rows, the rest right."""
    from view_fusion_amd import _lib
    host, store = stores
    ids = torch.tensor([3, 4, 5], dtype=torch.int64, device=dev)
    objects = torch.tensor([2, N, -1], dtype=torch.int64, device=dev)
    y_0 = torch.zeros(3, 3, store.H, store.W, device=dev)
    y_cond = torch.zeros(3, 23, 3, store.H, store.W, device=dev)
    angle, used = torch.zeros(3, 1, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.call("vf_batch_assemble", p(store.views), N, store.H, store.W, SEED, p(ids), p(objects), 3, 1, 0, 0, p(y_0),
              p(y_cond), p(angle), p(used), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    pl = data_ref.plan(SEED, [3], True, 1, 6, N, [2])
    w0, wc, wa = data_ref.assemble(host, pl, False)
    assert np.array_equal(_u32(y_0[:1]), _u32(w0)) and np.array_equal(_u32(y_cond[:1]), _u32(wc))
    assert np.array_equal(_u32(angle[:1]), _u32(wa)) and used.tolist() == [2, N, -1]
    assert torch.isnan(y_0[1:]).all() and torch.isnan(y_cond[1:]).all() and torch.isnan(angle[1:]).all()


def test_store_offsets_are_64_bit(dev):
    """14 600 objects of 24 x 3 x 64 x 64 bytes: the last object starts beyond 2^32 bytes (and so beyond 2^31; 14 565
    objects is the least for which it does).  4.3 GB, uninitialised but for its first and last object."""
    from view_fusion_amd import data
    n = 14600
    per = 24 * 3 * 64 * 64
    assert (n - 1) * per > 2 ** 32 > 2 ** 31
    host = _bytes((2, 24, 3, 64, 64), 9)
    views = torch.empty(n, 24, 3, 64, 64, dtype=torch.uint8, device=dev)
    views[0].copy_(torch.from_numpy(host[0]))
    views[n - 1].copy_(torch.from_numpy(host[1]))
    store = data.ViewStore(views)
    assert store.views.data_ptr() == views.data_ptr()
    for relative in (False, True):
        batch = store.batch(SEED, [11, 12], objects=[n - 1, 0], relative=relative)
        pl = data_ref.plan(SEED, [11, 12], True, 1, 6, n, [n - 1, 0])
        _check(batch, host, dict(pl, object=np.array([1, 0])), relative)
    assert np.array_equal(_u32(store.all_views([n - 1])[0]), _u32(data_ref.pixels(host[1])))
    drawn = data_ref.plan(SEED, IDS, True, 1, 6, n)["object"]
    assert drawn.max() < n and drawn.max() > n // 2          # (drawn objects reach the far half of such a store)
    del store, views, batch
    torch.cuda.empty_cache()


# ---- integration ---------------------------------------------------------------------------------------------------------
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
HW = TINY["image_size"]


def _model(dev, sched=SCHED):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": sched}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


@pytest.fixture(scope="module")
def store16(dev):
    from view_fusion_amd import data
    host = _bytes((N, 24, 3, HW, HW), 16)
    return host, data.ViewStore(torch.from_numpy(host).to(dev))


@pytest.mark.parametrize("graph,max_views", [(False, 3), (True, 1)], ids=["eager", "graph"])
def test_draw_batch_is_the_restatements_batch_for_the_steps_ids(store16, dev, graph, max_views):
    """max_views = 1 in graph mode: every step then has the same stacked-view count, so the third step is a replay."""
    from view_fusion_amd import train
    host, store = store16
    B, seed = 4, 13
    tr_a = train.Trainer(_model(dev), lr_warmup=1, graph=graph, seed=seed)
    tr_b = train.Trainer(_model(dev), lr_warmup=1, graph=graph, seed=seed)
    for s in range(3):
        batch = tr_a.draw_batch(store, B, max_views=max_views)
        ids = train.step_sample_ids(tr_b.it + 1, B) + np.arange(B)
        pl = data_ref.plan(seed, ids, True, 1, max_views, N)
        y_0, y_cond, angle = data_ref.assemble(host, pl, False)
        ref = dict(y_0=torch.from_numpy(y_0).to(dev), y_cond=torch.from_numpy(y_cond).to(dev),
                   angle=torch.from_numpy(angle).to(dev), view_count=torch.from_numpy(pl["view_count"]))
        assert batch["view_count"].tolist() == ref["view_count"].tolist()
        la, lb = tr_a.step(batch), tr_b.step(ref)
        print(f"step {s}: ids {ids.tolist()} view_count {batch['view_count'].tolist()} loss {float(la):.7f} / {float(lb):.7f}")
        assert torch.isfinite(la) and torch.equal(la, lb)
    assert tr_a.graph_steps == tr_b.graph_steps == (1 if graph else 0)
    assert all(torch.equal(a, b) for a, b in zip(tr_a.module.parameters(), tr_b.module.parameters()))


def test_draw_batch_runs_with_accumulation(store16, dev):
    from view_fusion_amd import train
    _, store = store16
    tr = train.Trainer(_model(dev), lr_warmup=1, graph=False, seed=3, accum_steps=2)
    whole = train.Trainer(_model(dev), lr_warmup=1, graph=False, seed=3)
    la, lb = tr.step(tr.draw_batch(store, 4, max_views=3)), whole.step(whole.draw_batch(store, 4, max_views=3))
    print(f"accum_steps=2 loss {float(la):.7f}  undivided {float(lb):.7f}")
    assert torch.isfinite(la) and abs(float(la) - float(lb)) <= 1e-5 * abs(float(lb))
    with pytest.raises(ValueError):
        train.Trainer(_model(dev), graph=False).draw_batch(store, 4)


def test_eval_batches_do_not_depend_on_the_batch_size(store16, dev):
    """The batches are the same rows bit for bit at B = 2 and B = 3 (that is this feature); the sampled images of one
    chain under two batchings agree to CHAIN_TOL max-abs, which moves an image's PSNR = -20 log10(rmse) by at
    most 20 / ln 10 * CHAIN_TOL / rmse; the bound below takes rmse from the smaller of the two mean PSNRs."""
    from view_fusion_amd import drivers
    host, store = store16
    vf = _model(dev, SCHED_C1)
    rows = {}
    for B in (2, 3):
        got = list(store.eval_batches(B, 5, max_views=3))
        assert [b["target"].shape[0] for b in got] == ([2, 2, 1] if B == 2 else [3, 2])
        rows[B] = {k: torch.cat([b[k] for b in got]) for k in ("target", "cond", "angle", "view_count", "ids")}
    for k in rows[2]:
        assert torch.equal(rows[2][k], rows[3][k]), k
    assert rows[2]["ids"].tolist() == list(range(N))
    pl = data_ref.plan(5, range(N), False, 1, 3, N, range(N))
    y_0, y_cond, angle = data_ref.assemble(host, pl, False)
    assert np.array_equal(_u32(rows[2]["target"]), _u32(y_0)) and np.array_equal(_u32(rows[2]["cond"]), _u32(y_cond))
    assert np.array_equal(_u32(rows[2]["angle"]), _u32(angle)) and rows[2]["view_count"].tolist() == pl["view_count"].tolist()
    shard = [b["ids"].tolist() for b in store.eval_batches(2, 5, rank=1, world=2)]
    assert shard == [[1, 3]]
    psnr = {B: float(drivers.evaluate(vf, store.eval_batches(B, 5, max_views=3), seed=5, sample_steps=2)["psnr"])
            for B in (2, 3)}
    bound = 20 / np.log(10) * CHAIN_TOL / 10 ** (-min(psnr.values()) / 20)
    print(f"psnr B=2 {psnr[2]:.6f}  B=3 {psnr[3]:.6f}  |diff| {abs(psnr[2] - psnr[3]):.3e}  bound {bound:.3e}")
    assert np.isfinite(psnr[2]) and abs(psnr[2] - psnr[3]) <= bound
