"""Seeded residual-block Dropout on the GPU (ops.dropout_seeded, dropout_seeded_kernel of csrc/elementwise.hip, the
drop_rng= of UNet.forward, ViewFusion.forward(seed=) and train.Trainer(seed=)).

  * the kernel against the numpy restatement tests/dropout_ref.py: mask and values bit for bit, forward and backward,
    into a NaN-filled buffer with guard words on either side;
  * bit-equal to the existing path (ops.dropout) fed u = k 2^-24, for a layer and for a whole UNet (output, x.grad and
    every parameter gradient);
  * a seeded ViewFusion step against the float64 oracle with the restated masks, and again with the batch permuted: the
    masks follow the sample ids, not the rows (stated tolerances: loss rel 1e-5, per-tensor gradient rel-L2 1e-4);
  * graph replay == eager bit for bit; accum_steps = 2 against the undivided batch under the existing bound
    |g_A - g_1| <= 4 e + 1e-7 max|g_1|, e MEASURED as the A = 1 gradient's distance from the float64 oracle;
  * nothing activation-sized is saved; the default paths launch what they launched; the refusals come before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch

import dropout_ref
from conftest import MICRO, TINY

pytestmark = pytest.mark.gpu
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
SEED = 0xC0FFEE1234567
IDS = [7, 2 ** 32 + 5, 1000003]          # not consecutive, one above 2^32
OFF = [0, 1, 4, 6]                       # view_count = [1, 3, 2]
P = 0.25                                 # exact in fp32 and in the oracle's float64 alike
GUARD = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev_rng(dev, ids, off):
    return (torch.tensor(ids, dtype=torch.int64, device=dev), torch.tensor(off, dtype=torch.int32, device=dev))


class _Spy:
    """Names of the C-ABI launches, in order (monkeypatched over _lib.call)."""

    def __init__(self, monkeypatch):
        from view_fusion_amd import _lib
        self.names, real = [], _lib.call

        def spy(name, *args):
            self.names.append(name)
            return real(name, *args)

        monkeypatch.setattr(_lib, "call", spy)

    def take(self):
        out, self.names[:] = list(self.names), []
        return out


# ---- 5. the kernel against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1036])       # 1036 = 259 float4: a second 256-thread block, partial
@pytest.mark.parametrize("layer", [0, 37])
def test_kernel_equals_the_restatement(dev, layer, n):
    from view_fusion_amd import _lib, ops
    S, p = OFF[-1], 0.3
    ids, off = _dev_rng(dev, IDS, OFF)
    x = np.random.default_rng(n + layer).standard_normal((S, n)).astype(np.float32)
    x[x == 0] = 1.0                                            # a zero in y is a dropped element, nothing else
    want_keep = dropout_ref.keep(SEED, IDS, OFF, n, p, layer)
    want = dropout_ref.apply(x, SEED, IDS, OFF, p, layer)
    # the launch through the C ABI into NaN: every element written, nothing outside
    thr, scale = ops.dropout_constants(p)
    xd = torch.from_numpy(x).to(dev)
    buf = torch.full((GUARD + S * n + GUARD,), float("nan"), device=dev)
    y = buf[GUARD:GUARD + S * n]
    assert y.data_ptr() % 16 == 0
    _lib.call("vf_dropout_seeded", ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(y.data_ptr()), SEED,
              ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(off.data_ptr()), len(IDS), S, n, thr, scale, layer,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    got = buf.cpu().numpy()
    assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + S * n:]).all()
    got = got[GUARD:GUARD + S * n].reshape(S, n)
    assert not np.isnan(got).any()
    assert np.array_equal(got != 0, want_keep) and np.array_equal(_bits(got), _bits(want))
    # the op: forward and backward (the same mask on dy)
    xt = xd.clone().requires_grad_(True)
    yt = ops.dropout_seeded(xt, p, SEED, ids, off, layer)
    assert np.array_equal(_bits(yt.detach().cpu().numpy()), _bits(want))
    dy = np.random.default_rng(99).standard_normal((S, n)).astype(np.float32)
    yt.backward(torch.from_numpy(dy).to(dev))
    assert np.array_equal(_bits(xt.grad.cpu().numpy()), _bits(dropout_ref.apply(dy, SEED, IDS, OFF, p, layer)))


def test_the_launcher_refuses_what_the_header_says(dev):
    from view_fusion_amd import _lib
    ids, off = _dev_rng(dev, IDS, OFF)
    x = torch.zeros(6, 8, device=dev)
    y = torch.full((6, 8), 5.0, device=dev)
    raw = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(n=8, thr=5, layer=0):
        _lib.call("vf_dropout_seeded", ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), SEED,
                  ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(off.data_ptr()), 3, 6, n, thr, 1.0, layer, raw)

    for bad in (dict(n=6), dict(thr=2 ** 24 + 1), dict(layer=65536), dict(layer=-1), dict(n=4 * 2 ** 32)):
        with pytest.raises(_lib.VFHipError):
            launch(**bad)
    assert bool((y == 5.0).all())                              # refused before the launch


# ---- 6. equals the existing path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_equals_the_existing_kernel_fed_the_same_uniforms(dev, p):
    from view_fusion_amd import ops
    S, n, layer = OFF[-1], 1036, 5
    ids, off = _dev_rng(dev, IDS, OFF)
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(S, n, generator=g).to(dev), torch.randn(S, n, generator=g).to(dev)
    u = torch.from_numpy(dropout_ref.uniforms(SEED, IDS, OFF, n, layer)).to(dev)
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = ops.dropout(a, p, u=u), ops.dropout_seeded(b, p, SEED, ids, off, layer)
    ya.backward(dy)
    yb.backward(dy)
    assert torch.equal(ya, yb) and torch.equal(a.grad, b.grad)
    kept = float((yb != 0).float().mean())
    assert abs(kept - (1 - p)) < 0.03                          # (6216 draws: 5 sigma at p = 0.5 is 0.032)


# ---- 7. a whole UNet -----------------------------------------------------------------------------------------------------
def _unet(dev, hp):
    from view_fusion_amd import UNet
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**hp)
    deterministic_fill_(net.state_dict())
    return net.to(dev)


def _layer_shapes(net, H, W):
    """(C, H, W) of the activation each residual block's Dropout sees, in execution order."""
    from view_fusion_amd.unet import _ResAttnBlock
    out = []
    for m in list(net.downs) + list(net.mid) + list(net.ups):
        if isinstance(m, _ResAttnBlock):
            conv = m.res_block.block2["block"]["3"]
            lvl = conv._vf_geom[0]
            out.append((conv.weight.shape[1], H >> lvl, W >> lvl))
            assert m.res_block._vf_layer == len(out) - 1
    return out


def _uniforms(net, seed, ids, off, H, W, dtype=torch.float32):
    S = off[-1]
    return [torch.from_numpy(dropout_ref.uniforms(seed, ids, off, c * h * w, layer).reshape(S, c, h, w)).to(dtype)
            for layer, (c, h, w) in enumerate(_layer_shapes(net, H, W))]


def test_whole_unet_equals_the_injected_uniforms(dev):
    net = _unet(dev, dict(TINY, dropout=P)).train()
    ids_l, off_l = [2 ** 32 + 5, 9], [0, 1, 3]                 # S = 3 from view_count = [1, 2]
    ids, off = _dev_rng(dev, ids_l, off_l)
    g = torch.Generator().manual_seed(5)
    x0, angle, level = torch.randn(3, 6, 16, 16, generator=g).to(dev), torch.rand(3, 1, generator=g).to(dev), \
        torch.rand(3, 1, generator=g).to(dev)
    dy = torch.randn(3, 6, 16, 16, generator=g).to(dev)
    us = [u.to(dev) for u in _uniforms(net, SEED, ids_l, off_l, 16, 16)]
    assert len(us) == 8

    def run(**kw):
        net.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = net(x, angle, level, **kw)
        y.backward(dy)
        return y.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in net.named_parameters()}

    ya, xa, ga = run(dropout_u=us)
    yb, xb, gb = run(drop_rng=(SEED, ids, off))
    assert torch.equal(ya, yb) and torch.equal(xa, xb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    # the masks took part, and an injected dropout_u wins over drop_rng
    net.eval()
    with torch.no_grad():
        y_eval = net(x0, angle, level)
    assert not torch.equal(y_eval, ya)
    net.train()
    yc, _, _ = run(dropout_u=[torch.ones_like(u) for u in us], drop_rng=(SEED, ids, off))
    assert not torch.equal(yc, ya)
    # the no-grad training-mode forward (the general path) draws the same masks
    with torch.no_grad():
        yn = net(x0, angle, level, drop_rng=(SEED, ids, off))
        assert torch.equal(yn, net(x0, angle, level, dropout_u=us))
    assert not torch.equal(yn, y_eval)


# ---- 8. batch invariance against the float64 oracle ---------------------------------------------------------------------
def _vf(dev, hp):
    from view_fusion_amd import ViewFusion
    vf = ViewFusion(_unet(dev, hp), {"train": dict(SCHED)}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


def _oracle64(vf, hp, seed, ids, batch, hw):
    """Loss and gradients of the float64 oracle on the device's drawn t, u and noise and the restated Dropout masks."""
    from oracle import unet_ref, view_fusion_ref as vfr
    from view_fusion_amd import ops
    dev = batch["y_0"].device
    ids_d = torch.as_tensor(ids, dtype=torch.int64).to(dev)
    vc = [int(v) for v in batch["view_count"]]
    off = [0] + list(np.cumsum(vc))
    t, _, u = ops.draw_train(seed, ids_d, vf.gammas, want_u=True)
    noise = ops.randn_ids(seed, ids_d, ops.diffusion.RNG_TRAIN_NOISE, 0, (3, hw, hw))
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in vf.denoise_fn.state_dict().items()}
    buf = {k: v.double() for k, v in vfr.schedule_buffers(vfr.beta_schedule(**SCHED)).items()}
    assert torch.equal(buf["gammas"].float(), vf.gammas.cpu())
    us = _uniforms(vf.denoise_fn, seed, [int(i) for i in ids], off, hw, hw, torch.float64)
    fn = lambda x, a, l: unet_ref.unet_forward(sd, hp, x, a, l, dropout_u=us)
    ref = vfr.train_loss(fn, buf, batch["y_cond"].cpu().double(), vc, batch["angle"].cpu().double(),
                         batch["y_0"].cpu().double(), t.cpu(), u.cpu().double().reshape(-1, 1), noise.cpu().double(), True)
    ref.backward()
    return float(ref.detach()), {k: v.grad for k, v in sd.items()}


def test_batch_invariance_against_the_float64_oracle(dev):
    from view_fusion_amd import train
    hp = dict(MICRO, dropout=P)
    vc, ids = [1, 3, 2], list(IDS)
    batch = dict(train.synthetic_batch(3, 3, 16, dev, seed=21), view_count=torch.tensor(vc))
    losses = []
    for perm in ([0, 1, 2], [2, 0, 1]):
        vf = _vf(dev, hp).train()
        b = dict(y_0=batch["y_0"][perm], y_cond=batch["y_cond"][perm], angle=batch["angle"][perm],
                 view_count=torch.tensor([vc[i] for i in perm]))
        pid = [ids[i] for i in perm]
        loss = vf(**b, seed=SEED, sample_ids=torch.tensor(pid, device=dev))
        loss.backward()
        lref, gref = _oracle64(vf, hp, SEED, pid, b, 16)
        print(f"perm {perm}: loss {loss.item():.9g}  oracle f64 {lref:.12g}  rel {abs(loss.item() - lref) / abs(lref):.3e}")
        assert abs(loss.item() - lref) <= 1e-5 * abs(lref), (perm, loss.item(), lref)
        worst, wk, compared = 0.0, None, 0
        for k, p in vf.denoise_fn.named_parameters():
            a, r = p.grad.detach().cpu().double(), gref[k]
            if float(r.norm()) > 1e-4:
                compared += 1
                err = float((a - r).norm() / r.norm())
                if err > worst:
                    worst, wk = err, k
        print(f"perm {perm}: worst gradient rel-L2 {worst:.3e} ({wk}) over {compared} tensors")
        assert compared >= len(gref) // 2 and worst < 1e-4, (perm, worst, wk, compared)
        losses.append(lref)
    # the permuted batch IS the same batch: the oracle, fed masks keyed by sample id, gives the same loss
    assert abs(losses[0] - losses[1]) <= 1e-12 * abs(losses[0])


# ---- 9. / 10. the Trainer ------------------------------------------------------------------------------------------------
TB, TN, TSEED = 4, 3, 11
TVC = [1, 3, 2, 2]
THP = dict(TINY, dropout=P)


def _trainer(dev, graph, **kw):
    from view_fusion_amd import train
    vf = _vf(dev, THP)
    tr = train.Trainer(vf, lr_warmup=1, graph=graph, seed=TSEED, **kw)
    tr.it = 0
    return vf, tr


def _tbatch(dev, s=0, vc=TVC):
    from view_fusion_amd import train
    return dict(train.synthetic_batch(TB, TN, 16, dev, seed=40 + s), view_count=torch.tensor(vc))


def _grads(vf):
    return [p.grad.detach().cpu().numpy().copy() for p in vf.parameters()]


def test_graph_replay_equals_eager(dev):
    """Steps 1-2 run eagerly, step 3 is captured and replayed, steps 4-5 replay that graph with other sample ids (every
    iteration has its own) and, in step 5, other view counts of the same sum: the captured forward AND backward must read
    the graph's own ids and offsets buffers, or the parameters part ways."""
    (vf_e, tr_e), (vf_g, tr_g) = _trainer(dev, False), _trainer(dev, True)
    for s in range(5):
        vc = TVC if s < 4 else [2, 2, 1, 3]
        le, lg = tr_e.step(_tbatch(dev, s, vc)), tr_g.step(_tbatch(dev, s, vc))
        torch.cuda.synchronize()
        assert torch.equal(le, lg), s
        for (k, a), b in zip(vf_e.named_parameters(), vf_g.parameters()):
            assert torch.equal(a, b), (s, k)
    assert tr_e.graph_steps == 0 and tr_g.graph_steps == 3 and len(tr_g._graphs) == 1 and tr_g.mode == "graph"
    # the step is not the step of a model without Dropout
    vf_0, tr_0 = _trainer(dev, False)
    for m in vf_0.modules():
        if hasattr(m, "_drop"):
            m.dropout = 0.0
    assert not torch.equal(tr_0.step(_tbatch(dev, 0)), _trainer(dev, False)[1].step(_tbatch(dev, 0)))


@pytest.fixture(scope="module")
def undivided(dev):
    """The undivided seeded Dropout batch (A = 1): its GPU gradient and loss, and the float64 oracle's with the restated
    masks and the device's draws.  Computed once; nothing below changes it."""
    from view_fusion_amd import train
    batch = _tbatch(dev)
    vf, tr = _trainer(dev, False)
    loss = float(tr.step(batch))
    names, g1 = [k for k, _ in vf.named_parameters()], _grads(vf)
    ids = (torch.arange(TB, dtype=torch.int64) + train.step_sample_ids(1, TB)).tolist()
    loss64, gref = _oracle64(_vf(dev, THP), THP, TSEED, ids, batch, 16)
    g64 = [gref[k[len("denoise_fn."):]].numpy() for k in names]
    e = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(g1, g64)]
    return dict(batch=batch, names=names, g1=g1, loss=loss, e=e, e_loss=abs(loss - loss64), loss64=loss64)


def test_accumulated_gradient_matches_the_undivided_batch(dev, undivided):
    r = undivided
    assert abs(r["loss"] - r["loss64"]) <= 1e-5 * abs(r["loss64"])          # (the A = 1 step is the oracle's step)
    vf, tr = _trainer(dev, False, accum_steps=2)
    loss = float(tr.step(r["batch"]))
    got = _grads(vf)
    worst = (0.0, None)
    for k, g, g1, e in zip(r["names"], got, r["g1"], r["e"]):
        diff, bound = float(np.abs(g.astype(np.float64) - g1).max()), 4.0 * e + 1e-7 * float(np.abs(g1).max())
        worst = max(worst, (diff / bound if bound else float(diff > 0), k))
    bound = 4.0 * r["e_loss"] + 1e-7 * abs(r["loss"])
    print(f"A=2 loss {loss:.9g}  A=1 {r['loss']:.9g}  oracle f64 {r['loss64']:.12g}  e {r['e_loss']:.3e}  "
          f"|diff| {abs(loss - r['loss']):.3e}  bound {bound:.3e};  worst gradient diff / bound {worst[0]:.3f} ({worst[1]})")
    for k, g, g1, e in zip(r["names"], got, r["g1"], r["e"]):
        assert float(np.abs(g.astype(np.float64) - g1).max()) <= 4.0 * e + 1e-7 * float(np.abs(g1).max()), k
    assert abs(loss - r["loss"]) <= bound


# ---- 11. nothing activation-sized is saved -------------------------------------------------------------------------------
def test_nothing_is_saved_for_backward(dev):
    net = _unet(dev, THP).train()
    blk = net.downs[1].res_block
    blk._vf_layer = 3
    S, C, H = OFF[-1], 32, 16
    ids, off = _dev_rng(dev, IDS, OFF)
    g = torch.Generator().manual_seed(2)
    x, e = torch.randn(S, C, H, H, generator=g).to(dev), torch.randn(S, C, generator=g).to(dev)
    u = torch.from_numpy(dropout_ref.uniforms(SEED, IDS, OFF, C * H * H, 3).reshape(S, C, H, H)).to(dev)

    def saved(**kw):
        seen = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (seen.append(t), t)[1], lambda t: t):
            y = blk(x.clone().requires_grad_(True), e, **kw)
        fl = sum(t.numel() * t.element_size() for t in seen if t.is_floating_point())
        it = sum(t.numel() * t.element_size() for t in seen if not t.is_floating_point())
        return y, fl, it

    ya, fa, ia = saved(draws=iter([u]))
    yb, fb, ib = saved(rng=(SEED, ids, off))
    assert torch.equal(ya, yb)
    a_bytes = S * C * H * H * 4
    print(f"saved floats: injected u {fa} B, seeded {fb} B, one activation {a_bytes} B; seeded ints {ib - ia} B")
    assert fa - fb == a_bytes
    assert ib - ia == ids.numel() * 8 + off.numel() * 4        # ids and off: 40 bytes here


# ---- 12. the defaults are unchanged --------------------------------------------------------------------------------------
def _vbatch(dev):
    from view_fusion_amd import train
    return dict(train.synthetic_batch(3, 3, 16, dev, seed=21), view_count=torch.tensor([1, 3, 2]))


def _kwargs_seen(net):
    seen = []
    h = net.register_forward_pre_hook(lambda m, a, kw: seen.append(dict(kw)), with_kwargs=True)
    return seen, h


def test_defaults_are_unchanged(dev, monkeypatch):
    spy = _Spy(monkeypatch)
    batch = _vbatch(dev)
    # dropout = 0 with seed=: the launches of a model that never heard of drop_rng, and no new keyword
    vf = _vf(dev, TINY).train()
    seen, h = _kwargs_seen(vf.denoise_fn)
    for _ in range(2):                                         # (the second forward: the weight-pack plans exist)
        vf.zero_grad()
        vf(**batch, seed=SEED).backward()
        names0 = spy.take()
        assert "vf_dropout_seeded" not in names0 and "vf_dropout" not in names0
    assert seen == [{}, {}]
    h.remove()
    # dropout > 0 without seed=: vf_dropout as before, once per residual block and direction
    vf = _vf(dev, THP).train()
    seen, h = _kwargs_seen(vf.denoise_fn)
    vf(**batch).backward()
    names = spy.take()
    assert names.count("vf_dropout") == 16 and "vf_dropout_seeded" not in names and seen == [{}]
    # ... with seed=: the seeded launch in its place, nothing else different
    vf.zero_grad()
    vf(**batch, seed=SEED).backward()
    seeded = spy.take()
    assert seeded.count("vf_dropout_seeded") == 16 and "vf_dropout" not in seeded
    assert set(seen[1]) == {"drop_rng"} and seen[1]["drop_rng"][0] == SEED
    assert [n for n in seeded if n != "vf_dropout_seeded"] == names0
    # eval mode: neither
    vf.eval()
    with torch.no_grad():
        vf(**batch, seed=SEED)
    names = spy.take()
    assert "vf_dropout" not in names and "vf_dropout_seeded" not in names and seen[-1] == {}
    h.remove()

    # a foreign denoise_fn with the three-argument signature trains with seed=
    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.full((1,), 0.5))

        def forward(self, x, angle, level):
            return x * self.w

    from view_fusion_amd import ViewFusion
    vf = ViewFusion(Stub().to(dev), {"train": dict(SCHED)}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    vf.train()
    loss = vf(**batch, seed=SEED)
    loss.backward()
    assert torch.isfinite(loss) and vf.denoise_fn.w.grad is not None and "vf_dropout_seeded" not in spy.take()


def test_distillation_student_draws_seeded_masks(dev, monkeypatch):
    teacher, student = _vf(dev, TINY), _vf(dev, THP)
    student.set_distill(teacher, steps=4)
    student.train()
    spy = _Spy(monkeypatch)
    seen, h = _kwargs_seen(student.denoise_fn)
    batch = _vbatch(dev)
    ids = torch.tensor(IDS, device=dev)
    la = student(**batch, seed=SEED, sample_ids=ids)
    la.backward()
    names = spy.take()
    h.remove()
    assert names.count("vf_dropout_seeded") == 16 and "vf_dropout" not in names
    assert len(seen) == 1 and torch.equal(seen[0]["drop_rng"][1], ids)      # (the teacher is another module, in eval mode)
    student.zero_grad()
    assert torch.equal(student(**batch, seed=SEED, sample_ids=ids), la)     # a function of (seed, ids): the same again


# ---- 13. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(dev, monkeypatch):
    from view_fusion_amd import ops
    spy = _Spy(monkeypatch)
    ids, off = _dev_rng(dev, [1], [0, 4096])
    x = torch.zeros(4096, 4, device=dev)
    with pytest.raises(ValueError, match="4096 views"):
        ops.dropout_seeded(x, 0.5, SEED, ids, off, 0)
    with pytest.raises(ValueError, match="4096 views"):
        ops.dropout_seeded(x, 0.5, SEED, ids, off, 0, max_views=4096)
    ids, off = _dev_rng(dev, IDS, OFF)
    with pytest.raises(ValueError, match="layer"):
        ops.dropout_seeded(torch.zeros(6, 4, device=dev), 0.5, SEED, ids, off, 65536)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.dropout_seeded(torch.zeros(6, 6, device=dev), 0.5, SEED, ids, off, 0)
    assert spy.take() == []
    # the largest numbering that is allowed runs: 4095 views, layer 65535
    ids, off = _dev_rng(dev, [1], [0, 4095])
    y = ops.dropout_seeded(torch.ones(4095, 4, device=dev), 0.5, SEED, ids, off, 65535)
    want = dropout_ref.apply(np.ones((4095, 4), dtype=np.float32), SEED, [1], [0, 4095], 0.5, 65535)
    assert np.array_equal(y.cpu().numpy(), want) and spy.take() == ["vf_dropout_seeded"]
