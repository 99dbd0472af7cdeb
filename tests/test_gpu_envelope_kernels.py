"""General-geometry kernels (csrc/conv_any.hip, csrc/norm_any.hip) on a real MI355X against torch-CPU fp32: direct
convolution at map sizes the specialised kernels refuse (non-square, non-power-of-two, 4x4, 256x256) in every mode,
forward / dgrad / wgrad with the epilogue operands, split-K on (S = 1) and off (S = 96); GroupNorm(+Swish) forward /
backward at any H*W; the bias / row-sum helpers on rows whose length is not a multiple of 4; run-to-run bitwise equality.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (4, 4), (5, 5), (6, 10), (12, 20), (24, 40), (48, 64), (64, 32), (96, 72), (256, 256)]
# S = 1: split-K on (the sampler regime); S = 96: split-K off (training grids) -- on the maps whose CPU reference is cheap
CONV_CASES = [(hw, 1) for hw in SHAPES] + [(hw, 96) for hw in SHAPES[:7]]
# GroupNorm: the shapes the register-resident kernels refuse (H*W not a power of two; a 256x256 group of 4 channels)
GN_SHAPES = [(1, 1), (5, 5), (6, 10), (12, 20), (24, 40), (48, 64), (96, 72), (256, 256)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _channels(H, W, S):
    # keep the CPU reference affordable on the big grids
    return (S, 32, 64) if (S > 8 or H * W >= 256 * 256) else (S, 96, 64)


def _conv_case(dev, H, W, S, KS, mode, Cin, Cout, epilogue, seed=0):
    """-> (GPU outputs, CPU outputs): y, dx, dw, db, dvb, dres for a conv whose OUTPUT is H x W."""
    from view_fusion_amd import ops
    g = torch.Generator().manual_seed(seed)
    Hi, Wi = {"same": (H, W), "down2": (2 * H, 2 * W), "up2": (H // 2, W // 2)}[mode]
    layer = torch.nn.Conv2d(Cin, Cout, KS, stride=2 if mode == "down2" else 1, padding=KS // 2)
    with torch.no_grad():
        layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) / (Cin * KS * KS) ** 0.5)
        layer.bias.copy_(torch.randn(Cout, generator=g) * 0.1)
    x = torch.randn(S, Cin, Hi, Wi, generator=g)
    vb = torch.randn(S, Cout, generator=g) if epilogue else None
    res = torch.randn(S, Cout, H, W, generator=g) if epilogue else None
    gy = torch.randn(S, Cout, H, W, generator=g)

    # CPU reference
    xc = x.clone().requires_grad_(True)
    lc = torch.nn.Conv2d(Cin, Cout, KS, stride=2 if mode == "down2" else 1, padding=KS // 2)
    lc.load_state_dict(layer.state_dict())
    vbc = vb.clone().requires_grad_(True) if epilogue else None
    resc = res.clone().requires_grad_(True) if epilogue else None
    xin = F.interpolate(xc, scale_factor=2, mode="nearest") if mode == "up2" else xc
    yc = lc(xin)
    if epilogue:
        yc = yc + vbc[:, :, None, None] + resc
    (yc * gy).sum().backward()

    lg = layer.to(dev)
    xg = x.to(dev).requires_grad_(True)
    vbg = vb.to(dev).requires_grad_(True) if epilogue else None
    resg = res.to(dev).requires_grad_(True) if epilogue else None
    yg = ops.conv2d(xg, lg, view_bias=vbg, residual=resg, mode=mode)
    (yg * gy.to(dev)).sum().backward()
    torch.cuda.synchronize()
    gpu = [yg, xg.grad, lg.weight.grad, lg.bias.grad] + ([vbg.grad, resg.grad] if epilogue else [])
    cpu = [yc, xc.grad, lc.weight.grad, lc.bias.grad] + ([vbc.grad, resc.grad] if epilogue else [])
    return [t.detach().cpu().clone() for t in gpu], cpu


def _modes(H, W):
    out = [(3, "same"), (1, "same"), (3, "down2")]
    if H % 2 == 0 and W % 2 == 0:
        out.append((3, "up2"))
    return out


@pytest.mark.parametrize("hw,S", CONV_CASES, ids=[f"{h}x{w}-S{s}" for (h, w), s in CONV_CASES])
def test_conv_any_geometry_vs_cpu(dev, hw, S):
    """Forward (modes same / down2 / up2), dgrad (mode 4 for down2) and wgrad, with and without the epilogue operands."""
    H, W = hw
    S, Cin, Cout = _channels(H, W, S)
    for KS, mode in _modes(H, W):
        for epi in (False, True):
            gpu, cpu = _conv_case(dev, H, W, S, KS, mode, Cin, Cout, epi)
            names = ["y", "dx", "dw", "db", "dvb", "dres"]
            for n, a, b in zip(names, gpu, cpu):
                assert rel(a, b) < 2e-5, (H, W, S, KS, mode, epi, n, rel(a, b))


@pytest.mark.parametrize("hw", [(5, 5), (6, 10), (24, 40), (96, 72)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_conv_any_is_bitwise_reproducible(dev, hw):
    H, W = hw
    for S in (1, 12):
        a, _ = _conv_case(dev, H, W, S, 3, "down2", 64, 64, True, seed=3)
        b, _ = _conv_case(dev, H, W, S, 3, "down2", 64, 64, True, seed=3)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.parametrize("hw", [(5, 5), (6, 10), (24, 40), (96, 72)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("S", [1, 24])
def test_conv1x1_cat_any_geometry(dev, hw, S):
    """The 1x1 conv on a never-materialised concatenation: forward, two-destination dgrad, wgrad."""
    from view_fusion_amd import ops
    from view_fusion_amd.ops.conv import _Conv1x1CatFn
    H, W = hw
    g = torch.Generator().manual_seed(5)
    C1, C2, Cout = 64, 96, 128
    layer = torch.nn.Conv2d(C1 + C2, Cout, 1)
    x1, x2 = torch.randn(S, C1, H, W, generator=g), torch.randn(S, C2, H, W, generator=g)
    gy = torch.randn(S, Cout, H, W, generator=g)
    a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    lc = torch.nn.Conv2d(C1 + C2, Cout, 1)
    lc.load_state_dict(layer.state_dict())
    yc = lc(torch.cat([a, b], 1))
    (yc * gy).sum().backward()
    lg = layer.to(dev)
    ag, bg = x1.to(dev).requires_grad_(True), x2.to(dev).requires_grad_(True)
    yg = _Conv1x1CatFn.apply(ag, bg, lg.weight, lg.bias, lg, True)
    (yg * gy.to(dev)).sum().backward()
    for n, p, q in (("y", yg, yc), ("dx1", ag.grad, a.grad), ("dx2", bg.grad, b.grad), ("dw", lg.weight.grad, lc.weight.grad),
                    ("db", lg.bias.grad, lc.bias.grad)):
        assert rel(p, q) < 2e-5, (hw, S, n, rel(p, q))
    with torch.no_grad():                      # the no-grad entry (the sampler) as well
        y2 = ops.conv1x1_cat(x1.to(dev), x2.to(dev), lg)
    assert rel(y2, yc) < 2e-5


@pytest.mark.parametrize("hw", GN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("silu", [False, True])
def test_group_norm_any_geometry_vs_cpu(dev, hw, silu):
    """GroupNorm(+Swish) forward / backward with the fused addend gradients (group_norm_skip), any H*W."""
    from view_fusion_amd import ops
    H, W = hw
    S, C, G = (1, 128, 32) if H * W >= 256 * 256 else (3, 96, 32)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(S, C, H, W, generator=g) * 2 + 0.5
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    gy, g1, g2 = (torch.randn(S, C, H, W, generator=g) for _ in range(3))
    xc, gc, bc = x.clone().requires_grad_(True), gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    yc = F.group_norm(xc, G, gc, bc, 1e-5)
    if silu:
        yc = F.silu(yc)
    ((yc * gy).sum() + (xc * g1).sum() + (xc * g2).sum()).backward()
    xg = x.to(dev).requires_grad_(True)
    gg, bg = gam.to(dev).requires_grad_(True), bet.to(dev).requires_grad_(True)
    yg, xs, xt = ops.group_norm_skip(xg, gg, bg, G, silu, tap=True)
    ((yg * gy.to(dev)).sum() + (xs * g1.to(dev)).sum() + (xt * g2.to(dev)).sum()).backward()
    for n, p, q in (("y", yg, yc), ("dx", xg.grad, xc.grad), ("dgamma", gg.grad, gc.grad), ("dbeta", bg.grad, bc.grad)):
        assert rel(p, q) < 2e-5, (hw, silu, n, rel(p, q))
    # plain GroupNorm (no addend) and a second run: bitwise equal
    outs = []
    for _ in range(2):
        xg = x.to(dev).requires_grad_(True)
        y = ops.group_norm(xg, gam.to(dev), bet.to(dev), G, silu)
        (y * gy.to(dev)).sum().backward()
        outs.append((y.detach().cpu(), xg.grad.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("HW", [1, 25, 35, 6913])
def test_bias_grad_and_rowsum_on_odd_rows(dev, HW):
    from view_fusion_amd.ops.core import _call, _ptr, _stream
    g = torch.Generator().manual_seed(HW)
    for S, C in ((5, 192), (3, 64)):
        dy = torch.randn(S, C, HW, generator=g)
        d = dy.to(dev)
        db = torch.empty(C, device=dev)
        dvb = torch.empty(S, C, device=dev)
        _call("vf_bias_grad", _ptr(d), _ptr(db), _ptr(dvb), S, C, HW, _stream())
        rows = torch.empty(S * C, device=dev)
        _call("vf_rowsum", _ptr(d), _ptr(rows), S * C, HW, _stream())
        ref = dy.double().sum(-1)
        np.testing.assert_allclose(dvb.cpu().double().numpy(), ref.numpy(), rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose(rows.cpu().double().numpy(), ref.reshape(-1).numpy(), rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose(db.cpu().double().numpy(), ref.sum(0).numpy(), rtol=1e-5, atol=1e-3)


def test_deferred_wgrad_main_and_multi_reduce_off_square(dev):
    """vf_conv_wgrad_main / vf_conv1x1_cat_wgrad_main at off-square shapes (the general weight-gradient kernel) with
    their slab sums in ONE vf_wino44_reduce_multi launch: equal to torch-CPU, and bitwise equal to the one-call
    vf_conv_wgrad / vf_conv1x1_cat_wgrad (same slabs, same reduce body)."""
    import ctypes
    from view_fusion_amd import _lib
    from view_fusion_amd.ops.core import _call, _ptr, _stream
    lib = _lib.load()
    g = torch.Generator().manual_seed(21)
    # (S, Cin, Cout, H, W (output), KS, mode, C1 for a 1x1 concatenated input)
    cases = [(4, 96, 64, 24, 40, 3, 0, 0), (3, 64, 128, 6, 10, 3, 1, 0), (2, 128, 64, 12, 20, 3, 2, 0),
             (5, 160, 64, 5, 5, 1, 0, 64)]
    rows, keep, first = [], [], 0
    for S, Cin, Cout, H, W, KS, m, C1 in cases:
        Hi, Wi = {0: (H, W), 1: (2 * H, 2 * W), 2: (H // 2, W // 2)}[m]
        x = torch.randn(S, Cin, Hi, Wi, generator=g)
        dy = torch.randn(S, Cout, H, W, generator=g)
        xc = x.clone().requires_grad_(True)
        w = torch.zeros(Cout, Cin, KS, KS, requires_grad=True)
        xin = F.interpolate(xc, scale_factor=2, mode="nearest") if m == 2 else xc
        (F.conv2d(xin, w, stride=2 if m == 1 else 1, padding=KS // 2) * dy).sum().backward()
        need = lib.vf_conv_wgrad_ws_floats(S, Cin, Cout, H, W, KS)
        ws = torch.empty(need, device=dev)
        ws1 = torch.empty(need, device=dev)
        dw = torch.empty(Cout, Cin, KS, KS, device=dev)
        dw1 = torch.empty_like(dw)
        xg, dyg = x.to(dev), dy.to(dev)
        row, nblk = (ctypes.c_longlong * 9)(), ctypes.c_int(0)
        rowp, nbp = ctypes.cast(row, ctypes.c_void_p), ctypes.cast(ctypes.pointer(nblk), ctypes.c_void_p)
        if C1:
            x1, x2 = xg[:, :C1].contiguous(), xg[:, C1:].contiguous()
            _call("vf_conv1x1_cat_wgrad_main", _ptr(x1), _ptr(x2), C1, _ptr(dyg), _ptr(dw), _ptr(ws), need, S, Cin, Cout,
                  H, W, rowp, nbp, _stream())
            _call("vf_conv1x1_cat_wgrad", _ptr(x1), _ptr(x2), C1, _ptr(dyg), _ptr(dw1), _ptr(ws1), need, S, Cin, Cout,
                  H, W, _stream())
            keep += [x1, x2]
        else:
            _call("vf_conv_wgrad_main", _ptr(xg), _ptr(dyg), _ptr(dw), _ptr(ws), need, S, Cin, Cout, H, W, KS, m, rowp,
                  nbp, _stream())
            _call("vf_conv_wgrad", _ptr(xg), _ptr(dyg), _ptr(dw1), _ptr(ws1), need, S, Cin, Cout, H, W, KS, m, _stream())
        assert nblk.value > 0
        r = list(row)
        r[8] = (r[8] & ~0xFFFFFFFF) | first            # `first` = the int32 at byte 64 of the row
        rows.append(r)
        first += nblk.value
        keep += [xg, dyg, ws, ws1]
        cases_out = (dw, dw1, w.grad)
        keep.append(cases_out)
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    _call("vf_wino44_reduce_multi", ctypes.c_void_p(table.data_ptr()), len(rows), first, _stream())
    torch.cuda.synchronize()
    outs = [k for k in keep if isinstance(k, tuple)]
    for (S, Cin, Cout, H, W, KS, m, C1), (dw, dw1, ref) in zip(cases, outs):
        assert rel(dw, ref) < 2e-5, (H, W, KS, m, rel(dw, ref))
        assert torch.equal(dw.cpu(), dw1.cpu()), (H, W, KS, m)
