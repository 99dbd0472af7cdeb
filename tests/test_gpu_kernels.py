"""Per-kernel parity on a real MI355X: every HIP launcher (through the C ABI / ops layer)
against the same op evaluated with stock fp32 PyTorch on the CPU.

Tolerance: fp32.  `rel` = max|a-b| / max|b|.  Contractions: 2e-5 forward / dgrad (K <= 5760),
1e-4 for weight gradients (K = S*H*W up to 2e4 here; different summation order); elementwise and
norm kernels 1e-5.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,HW,silu", [(64, 64, True), (128, 64, True), (192, 64, True), (256, 64, False),
                                       (320, 32, True), (256, 32, True), (192, 8, True), (640, 8, True),
                                       (512, 16, True), (32, 16, True), (192, 16, False), (96, 8, True)])
def test_group_norm_fwd_bwd(dev, C, HW, silu):
    from view_fusion_amd import ops
    S = 3
    x = rnd(S, C, HW, HW, seed=1) * 3 + 0.5
    ga, be = 1 + 0.2 * rnd(C, seed=2), 0.2 * rnd(C, seed=3)
    gy = rnd(S, C, HW, HW, seed=4)
    xc = x.clone().requires_grad_(True); gac = ga.clone().requires_grad_(True); bec = be.clone().requires_grad_(True)
    yc = F.group_norm(xc, 32, gac, bec, eps=1e-5)
    if silu:
        yc = yc * torch.sigmoid(yc)
    yc.backward(gy)
    xg = x.to(dev).requires_grad_(True); gag = ga.to(dev).requires_grad_(True); beg = be.to(dev).requires_grad_(True)
    yg = ops.group_norm(xg, gag, beg, 32, silu)
    yg.backward(gy.to(dev))
    assert rel(yg, yc) < 1e-5
    assert rel(xg.grad, xc.grad) < 2e-5
    assert rel(gag.grad, gac.grad) < 2e-5
    assert rel(beg.grad, bec.grad) < 2e-5


CONV_CASES = [
    # (Cin, Cout, H_in, KS, mode)
    (6, 64, 64, 3, "same"), (64, 64, 64, 3, "same"), (64, 6, 64, 3, "same"), (128, 128, 32, 3, "same"),
    (192, 192, 16, 3, "same"), (320, 320, 8, 3, "same"), (640, 320, 8, 3, "same"), (192, 128, 64, 3, "same"),
    (64, 64, 64, 3, "down2"), (128, 128, 32, 3, "down2"), (192, 192, 16, 3, "down2"),
    (320, 320, 8, 3, "up2"), (192, 192, 16, 3, "up2"), (128, 128, 32, 3, "up2"),
    (64, 128, 32, 1, "same"), (192, 576, 16, 1, "same"), (320, 960, 8, 1, "same"), (512, 192, 16, 1, "same"),
    (96, 64, 16, 1, "same"), (32, 32, 16, 3, "same"), (32, 32, 16, 3, "down2"), (64, 64, 8, 3, "up2"),
]


@pytest.mark.parametrize("Cin,Cout,Hin,KS,mode", CONV_CASES)
@pytest.mark.parametrize("S", [3])
def test_conv_fwd_bwd(dev, Cin, Cout, Hin, KS, mode, S, tol=2e-5):
    from view_fusion_amd import ops
    layer = torch.nn.Conv2d(Cin, Cout, KS, padding=KS // 2)
    with torch.no_grad():
        layer.weight.copy_(rnd(Cout, Cin, KS, KS, seed=5) / math.sqrt(Cin * KS * KS))
        layer.bias.copy_(rnd(Cout, seed=6) * 0.1)
    x = rnd(S, Cin, Hin, Hin, seed=7)
    Hout = Hin // 2 if mode == "down2" else (Hin * 2 if mode == "up2" else Hin)
    vb = rnd(S, Cout, seed=8) * 0.3
    res = rnd(S, Cout, Hout, Hout, seed=9)
    gy = rnd(S, Cout, Hout, Hout, seed=10)

    xc = x.clone().requires_grad_(True); vbc = vb.clone().requires_grad_(True); rc = res.clone().requires_grad_(True)
    inp = F.interpolate(xc, scale_factor=2, mode="nearest") if mode == "up2" else xc
    yc = F.conv2d(inp, layer.weight, layer.bias, stride=2 if mode == "down2" else 1, padding=KS // 2)
    yc = yc + vbc[:, :, None, None] + rc
    yc.backward(gy)
    wgc, bgc = layer.weight.grad.clone(), layer.bias.grad.clone()
    layer.zero_grad()

    layer = layer.to(dev)
    xg = x.to(dev).requires_grad_(True); vbg = vb.to(dev).requires_grad_(True); rg = res.to(dev).requires_grad_(True)
    yg = ops.conv2d(xg, layer, view_bias=vbg, residual=rg, mode=mode)
    yg.backward(gy.to(dev))
    assert rel(yg, yc) < tol
    assert rel(xg.grad, xc.grad) < tol
    assert rel(layer.weight.grad, wgc) < 1e-4
    assert rel(layer.bias.grad, bgc) < 2e-5
    assert rel(vbg.grad, vbc.grad) < 2e-5
    assert rel(rg.grad, rc.grad) < 1e-6


C11_CASES = [(192, 576, 16, 40), (576, 192, 16, 48), (128, 64, 64, 20), (64, 128, 64, 16), (320, 128, 32, 64),
             (192, 192, 16, 96), (96, 160, 8, 600), (32, 64, 32, 70), (640, 320, 8, 351)]


def test_conv1x1_training_size_kernel():
    """The dedicated 1x1 kernel of csrc/conv1x1.hip (weights straight from global memory, 128 x 128 tiles) -- forward with
    bias + per-view bias + residual and dgrad, incl. an odd number of 64-channel tiles (576 = 9, 160 -> 3, 320 = 5), a
    Cout below one tile, 8x8 maps (a 128-pixel tile spans two views) and a pixel count that is no multiple of 128 (351
    views of 8x8), plus the concatenated-input / split-output forms.  Its natural policy (deep K, even tile count, two
    workgroups per CU) is what the full-size model tests run; here VF_CONV1X1_FORCE=1 routes every legal shape to it --
    the library reads that variable once, so the cases run in a child process of their own."""
    import subprocess
    import sys
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r);"
            "import test_gpu_kernels as t; dev = torch.device('cuda:0');"
            "[t.test_conv_fwd_bwd(dev, ci, co, h, 1, 'same', s) for ci, co, h, s in t.C11_CASES];"
            "[t.test_cat_free_decoder_ops(dev, *c) for c in [(64, 64, 64, 64, 12), (192, 128, 32, 128, 40), (128, 64, 16, 192, 80)]];"
            "print('C11_OK')") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VF_CONV1X1_FORCE="1"), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "C11_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("Cin,Cout,Hin,KS,mode", [(320, 320, 8, 3, "same"), (64, 64, 64, 3, "same"),
                                                  (192, 576, 16, 1, "same"), (128, 128, 32, 3, "down2"),
                                                  (192, 192, 16, 3, "up2"), (640, 320, 8, 1, "same")])
def test_conv_small_batch_split_k_forward(dev, Cin, Cout, Hin, KS, mode, S):
    """Sampler regime: tiny grids take the split-K path (partials + reduce with the fused epilogue)."""
    test_conv_fwd_bwd(dev, Cin, Cout, Hin, KS, mode, S)


@pytest.mark.parametrize("Cin,Hin,S,use_tap", [(64, 64, 3, True), (128, 32, 2, True), (192, 16, 5, True), (32, 16, 3, False)])
def test_conv_down2_tap_adds_the_skip_gradient_in_the_dgrad_epilogue(dev, Cin, Hin, S, use_tap):
    """The encoder's stride-2 conv hands out a second handle on its input (the decoder's skip connection); the
    gradient arriving through it is added in the sub-pixel dgrad kernel's epilogue."""
    from view_fusion_amd import ops
    layer = torch.nn.Conv2d(Cin, Cin, 3, 2, 1)
    with torch.no_grad():
        layer.weight.copy_(rnd(Cin, Cin, 3, 3, seed=5) / math.sqrt(Cin * 9))
        layer.bias.copy_(rnd(Cin, seed=6) * 0.1)
    x = rnd(S, Cin, Hin, Hin, seed=7)
    gy, gt = rnd(S, Cin, Hin // 2, Hin // 2, seed=8), rnd(S, Cin, Hin, Hin, seed=9)
    xc = x.clone().requires_grad_(True)
    yc = F.conv2d(xc, layer.weight, layer.bias, stride=2, padding=1)
    ((yc * gy).sum() + ((xc * gt).sum() if use_tap else 0)).backward()
    wgc = layer.weight.grad.clone()
    layer.zero_grad()
    layer = layer.to(dev)
    xg = x.to(dev).requires_grad_(True)
    yg, xt = ops.conv2d(xg, layer, mode="down2", tap=True)
    ((yg * gy.to(dev)).sum() + ((xt * gt.to(dev)).sum() if use_tap else 0)).backward()
    assert rel(yg, yc) < 2e-5 and rel(xg.grad, xc.grad) < 2e-5 and rel(layer.weight.grad, wgc) < 1e-4


SMALL_CASES = [c for c in CONV_CASES if c[4] == "same" and c[0] % (4 if c[3] == 1 else 32) == 0] + [
    (64, 100, 16, 3, "same"), (32, 40, 4, 3, "same"), (68, 33, 8, 1, "same"), (96, 50, 8, 3, "same"),
    (384, 192, 16, 3, "same"), (512, 192, 16, 3, "same"), (256, 128, 32, 3, "same"), (192, 64, 64, 3, "same"),
    # round 5: the Upsample conv (nearest x2 folded into the patch addressing of the one-launch kernel)
    (128, 128, 32, 3, "up2"), (192, 192, 16, 3, "up2"), (64, 40, 4, 3, "up2"), (32, 64, 8, 3, "up2"),
    (64, 6, 64, 3, "same"), (64, 48, 64, 3, "same")]       # (fewer than 32 / an odd number of 16-row blocks under 32-channel workgroups)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("Cin,Cout,Hin,KS,mode", SMALL_CASES)
def test_conv_small_sampler_kernel(dev, Cin, Cout, Hin, KS, mode, S):
    """The sampler's one-launch conv (csrc/conv_small.hip: K split over the waves of a workgroup) against an fp64
    convolution, through the same ops.conv2d call the no-grad UNet forward makes: a 1x1 layer reads the unpacked OIHW
    parameter through vf_conv_small, a 3x3 layer the packed copy (vf_conv_small_pack, made once per weight version)
    through vf_conv_small_gn.  The unpacked 3x3 kernels run in tests/test_gpu_conv_small_plan.py."""
    from view_fusion_amd import ops
    layer = torch.nn.Conv2d(Cin, Cout, KS, padding=KS // 2)
    with torch.no_grad():
        layer.weight.copy_(rnd(Cout, Cin, KS, KS, seed=5) / math.sqrt(Cin * KS * KS))
        layer.bias.copy_(rnd(Cout, seed=6) * 0.1)
    x = rnd(S, Cin, Hin, Hin, seed=7)
    Hout = Hin // 2 if mode == "down2" else (Hin * 2 if mode == "up2" else Hin)
    vb, res = rnd(S, Cout, seed=8) * 0.3, rnd(S, Cout, Hout, Hout, seed=9)
    inp = F.interpolate(x.double(), scale_factor=2, mode="nearest") if mode == "up2" else x.double()
    ref = F.conv2d(inp, layer.weight.double(), layer.bias.double(), stride=2 if mode == "down2" else 1, padding=KS // 2)
    ref = ref + vb.double()[:, :, None, None] + res.double()
    layer = layer.to(dev)
    ops.st.KERNEL_LOG = []
    saved = ops.st.SMALL_CONV_MAX_WGS, ops.st.SMALL_CONV_MAX_CIN3, ops.st.SMALL_CONV_MAX_S3
    ops.st.SMALL_CONV_MAX_WGS, ops.st.SMALL_CONV_MAX_CIN3, ops.st.SMALL_CONV_MAX_S3 = (1 << 30, 1 << 30), 1 << 30, 1 << 30
    try:
        assert ops.use_small_conv(S, Cin, Cout, Hout, Hout, KS, ops._MODES[mode])
        with torch.no_grad():
            y = ops.conv2d(x.to(dev), layer, view_bias=vb.to(dev), residual=res.to(dev), mode=mode)
            y0 = ops.conv2d(x.to(dev), layer, mode=mode)
        torch.cuda.synchronize()
        # (3x3: the general entry with the packed weight copy, made once per weight version; 1x1: the plain entry)
        names = [e[5] for e in ops.st.KERNEL_LOG if e[5] != "vf_conv_small_pack"]
        assert names == (["vf_conv_small_gn"] * 2 if KS == 3 else ["vf_conv_small"] * 2), names
        assert sum(e[5] == "vf_conv_small_pack" for e in ops.st.KERNEL_LOG) == (1 if KS == 3 else 0)
    finally:
        ops.st.KERNEL_LOG = None
        ops.st.SMALL_CONV_MAX_WGS, ops.st.SMALL_CONV_MAX_CIN3, ops.st.SMALL_CONV_MAX_S3 = saved
    assert rel(y, ref) < 2e-6
    assert rel(y0, ref - vb.double()[:, :, None, None] - res.double()) < 2e-6


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("C,H,rC1,rC2", [(64, 64, 64, 64), (64, 64, 128, 64), (128, 32, 64, 0), (128, 32, 192, 128),
                                         (192, 16, 128, 0), (192, 16, 192, 192), (100, 8, 36, 0), (32, 4, 20, 12)])
def test_conv_small_with_folded_residual_conv(dev, C, H, rC1, rC2, S):
    """Round 5: a residual block's last 3x3 conv with the block's residual 1x1 conv folded in as extra K
    (vf_conv_small_res; reference unet.py:238,245: block2(h) + res_conv(x), x possibly the decoder's never-materialised
    concatenation) against fp64, through the ops.conv2d(..., res_fold=) call of the no-grad UNet forward."""
    from view_fusion_amd import ops
    Cin = C if C % 32 == 0 else 96          # (3x3 small kernel: Cin a multiple of 32; Cout free)
    conv, resc = torch.nn.Conv2d(Cin, C, 3, padding=1), torch.nn.Conv2d(rC1 + rC2, C, 1)
    with torch.no_grad():
        conv.weight.copy_(rnd(C, Cin, 3, 3, seed=5) / math.sqrt(Cin * 9))
        conv.bias.copy_(rnd(C, seed=6) * 0.1)
        resc.weight.copy_(rnd(C, rC1 + rC2, 1, 1, seed=15) / math.sqrt(rC1 + rC2))
        resc.bias.copy_(rnd(C, seed=16) * 0.1)
    a2, vb = rnd(S, Cin, H, H, seed=7), rnd(S, C, seed=8) * 0.3
    x1 = rnd(S, rC1, H, H, seed=9)
    x2 = rnd(S, rC2, H, H, seed=10) if rC2 else None
    xin = torch.cat([x1, x2], 1) if rC2 else x1
    ref = (F.conv2d(a2.double(), conv.weight.double(), conv.bias.double(), padding=1) + vb.double()[:, :, None, None]
           + F.conv2d(xin.double(), resc.weight.double(), resc.bias.double()))
    conv, resc = conv.to(dev), resc.to(dev)
    saved = ops.st.SMALL_CONV_MAX_WGS, ops.st.SMALL_CONV_MAX_CIN3, ops.st.SMALL_CONV_MAX_S3
    ops.st.SMALL_CONV_MAX_WGS, ops.st.SMALL_CONV_MAX_CIN3, ops.st.SMALL_CONV_MAX_S3 = (1 << 30, 1 << 30), 1 << 30, 1 << 30
    ops.st.KERNEL_LOG = []
    try:
        with torch.no_grad():
            fold = (resc, x1.to(dev), None if x2 is None else x2.to(dev))
            y = ops.conv2d(a2.to(dev), conv, view_bias=vb.to(dev), res_fold=fold)
            y_nb = ops.conv2d(a2.to(dev), conv, res_fold=fold)
        torch.cuda.synchronize()
        assert [e[5] for e in ops.st.KERNEL_LOG if e[5] != "vf_conv_small_pack"] == ["vf_conv_small_gn"] * 2   # (general entry: packed weights + fold)
    finally:
        ops.st.KERNEL_LOG = None
        ops.st.SMALL_CONV_MAX_WGS, ops.st.SMALL_CONV_MAX_CIN3, ops.st.SMALL_CONV_MAX_S3 = saved
    assert rel(y, ref) < 2e-6
    assert rel(y_nb, ref - vb.double()[:, :, None, None]) < 2e-6


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("C0,C1,C2,H,KS2", [(64, 64, 64, 64, 3), (128, 128, 64, 32, 3), (192, 192, 576, 16, 1),
                                            (64, 192, 192, 16, 3), (96, 320, 100, 8, 1), (32, 32, 40, 4, 3)])
def test_conv_small_groupnorm_without_a_launch(dev, C0, C1, C2, H, KS2, S):
    """conv -> GroupNorm(32)+Swish -> conv with NO GroupNorm launch (the optional statistics operands of
    vf_conv_small_gn): the first conv's epilogue accumulates per-(view, channel) integer sums of its output, the second
    conv normalises while staging -- against fp64 of the reference's Block chain (unet.py:207-218); the sums themselves
    against fp64 to 2^-24-unit fixed-point accuracy; bit-reproducible across launches (integer atomics).  The sampler
    does not take this route (round 5 measured it 4 % slower than a GroupNorm launch, profiles/r05_sampler.md; round 6
    removed the host path): the test drives the C ABI directly."""
    import ctypes
    from view_fusion_amd import _lib, ops
    conv1, conv2 = torch.nn.Conv2d(C0, C1, 3, padding=1), torch.nn.Conv2d(C1, C2, KS2, padding=KS2 // 2)
    gn = torch.nn.GroupNorm(32, C1)
    with torch.no_grad():
        conv1.weight.copy_(rnd(C1, C0, 3, 3, seed=5) / math.sqrt(C0 * 9))
        conv1.bias.copy_(rnd(C1, seed=6) * 0.5 + 0.7)               # (a mean well away from zero)
        conv2.weight.copy_(rnd(C2, C1, KS2, KS2, seed=7) / math.sqrt(C1 * KS2 * KS2))
        conv2.bias.copy_(rnd(C2, seed=8) * 0.1)
        gn.weight.copy_(1 + 0.3 * rnd(C1, seed=9))
        gn.bias.copy_(0.2 * rnd(C1, seed=10))
    x, vb = rnd(S, C0, H, H, seed=11), rnd(S, C1, seed=12) * 0.3
    silu = KS2 == 3
    h_ref = F.conv2d(x.double(), conv1.weight.double(), conv1.bias.double(), padding=1) + vb.double()[:, :, None, None]
    n_ref = F.group_norm(h_ref, 32, gn.weight.double(), gn.bias.double(), 1e-5)
    if silu:
        n_ref = n_ref * torch.sigmoid(n_ref)
    y_ref = F.conv2d(n_ref, conv2.weight.double(), conv2.bias.double(), padding=KS2 // 2)
    conv1, conv2, gn = conv1.to(dev), conv2.to(dev), gn.to(dev)
    xd, vbd = x.to(dev), vb.to(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st_raw = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def packed(conv):
        if conv.weight.shape[2] != 3 or conv.weight.shape[1] % 32:
            return None
        wp = torch.empty(_lib.load().vf_conv_small_pack_floats(conv.weight.shape[0], conv.weight.shape[1]), device=dev)
        _lib.call("vf_conv_small_pack", P(conv.weight.detach()), P(wp), conv.weight.shape[0], conv.weight.shape[1], st_raw)
        return wp

    def launch(xin, conv, view_bias, in_stats, out_stats):
        Cout, Cin, KS, _ = conv.weight.shape
        y = torch.empty(S, Cout, H, H, device=dev)
        wp = packed(conv)
        _lib.call("vf_conv_small_gn", P(xin), None, 0, P(conv.weight.detach()), P(conv.bias.detach()), P(view_bias), None, P(y), S,
                  Cin, Cout, H, H, KS, P(in_stats), P(gn.weight.detach()) if in_stats is not None else None,
                  P(gn.bias.detach()) if in_stats is not None else None, 32 if in_stats is not None else 0, 1e-5, int(silu),
                  P(out_stats), None, None, 0, 0, None, None, P(wp), 0, st_raw)
        return y

    outs = []
    for _ in range(2):
        st = torch.zeros(S * C1 * 2, dtype=torch.int64, device=dev)
        h = launch(xd, conv1, vbd, None, st)
        y = launch(h, conv2, None, st, None)
        outs.append((h.clone(), st.clone(), y.clone()))
    torch.cuda.synchronize()
    (h, st, y), (h2, st2, y2) = outs
    assert torch.equal(st, st2) and torch.equal(y, y2)                # order-independent sums: bit-reproducible
    assert rel(h, h_ref) < 2e-6
    sums = st.view(S, C1, 2).double().cpu() / 2.0 ** 24
    hd = h.double().cpu()
    np.testing.assert_allclose(sums[..., 0].numpy(), hd.sum(dim=(2, 3)).numpy(), rtol=1e-6, atol=2e-4)
    np.testing.assert_allclose(sums[..., 1].numpy(), (hd * hd).sum(dim=(2, 3)).numpy(), rtol=1e-6, atol=2e-4)
    assert rel(y, y_ref) < 5e-6, rel(y, y_ref)


@pytest.mark.parametrize("Cin,Cout,H,mode,S", [(128, 64, 64, "same", 6), (192, 64, 64, "same", 6), (128, 128, 32, "same", 6),
                                               (128, 128, 64, "up2", 3), (192, 192, 32, "up2", 6), (320, 128, 32, "same", 6),
                                               (256, 128, 32, "same", 12), (128, 192, 16, "same", 16), (70, 96, 32, "same", 12)])
def test_winograd_fixup_evaluates_the_groupnorm(dev, Cin, Cout, H, mode, S):
    """Round 5, the sampler at a few views: where every tile of the nested Winograd launch is a K-split tail tile the
    fix-up launch also evaluates the GroupNorm(+Swish) behind the conv (vf_wino_conv_fwd_gn) -- conv output and
    normalised output against fp64 of conv -> GroupNorm(32) -> Swish (reference unet.py:207-218), with bias, per-view
    bias and residual, with and without storing y."""
    from view_fusion_amd import ops
    layer, gn = torch.nn.Conv2d(Cin, Cout, 3, padding=1), torch.nn.GroupNorm(32, Cout)
    with torch.no_grad():
        layer.weight.copy_(rnd(Cout, Cin, 3, 3, seed=5) / math.sqrt(Cin * 9))
        layer.bias.copy_(rnd(Cout, seed=6) * 0.5 + 0.4)
        gn.weight.copy_(1 + 0.3 * rnd(Cout, seed=9))
        gn.bias.copy_(0.2 * rnd(Cout, seed=10))
    Hin = H // 2 if mode == "up2" else H
    x, vb, res = rnd(S, Cin, Hin, Hin, seed=7), rnd(S, Cout, seed=8) * 0.3, rnd(S, Cout, H, H, seed=11)
    inp = F.interpolate(x.double(), scale_factor=2, mode="nearest") if mode == "up2" else x.double()
    y_ref = F.conv2d(inp, layer.weight.double(), layer.bias.double(), padding=1) + vb.double()[:, :, None, None] + res.double()
    a_ref = F.group_norm(y_ref, 32, gn.weight.double(), gn.bias.double(), 1e-5)
    a_ref = a_ref * torch.sigmoid(a_ref)
    layer, gn = layer.to(dev), gn.to(dev)
    lib = ops._lib.load()
    m = ops._MODES[mode]
    with torch.no_grad():
        if not (ops.wino_kind(S, Cin, Cout, H, H, 3, m, False) == 1 and lib.vf_wino_conv_gn_fusable(S, Cin, Cout, H, H, m, 32)):
            pytest.skip("this shape does not take the fused fix-up at this S under the natural policy")
        ops.st.KERNEL_LOG = []
        try:
            y, a = ops.conv2d_gn(x.to(dev), layer, gn, 32, True, view_bias=vb.to(dev), residual=res.to(dev), mode=mode,
                                 want_y=True)
            y2, a2 = ops.conv2d_gn(x.to(dev), layer, gn, 32, True, view_bias=vb.to(dev), residual=res.to(dev), mode=mode)
            torch.cuda.synchronize()
            assert [e[5] for e in ops.st.KERNEL_LOG if e[5] != "vf_wino_pack_weights"] == ["vf_wino_conv_fwd_gn"] * 2
        finally:
            ops.st.KERNEL_LOG = None
    assert y2 is None and torch.equal(a, a2)
    assert rel(y, y_ref) < 2e-5 and rel(a, a_ref) < 2e-5, (rel(y, y_ref), rel(a, a_ref))


@pytest.mark.parametrize("S", [1, 4])
def test_conv_small_cat_and_gn(dev, S):
    """The decoder's 1x1 conv on the never-materialised concatenation, and conv + GroupNorm(+Swish) of the inference
    path, at sampler sizes (both route through the one-launch kernel)."""
    from view_fusion_amd import ops
    C1, C2, Cout, H = 128, 64, 96, 16
    layer = torch.nn.Conv2d(C1 + C2, Cout, 1)
    with torch.no_grad():
        layer.weight.copy_(rnd(Cout, C1 + C2, 1, 1, seed=5) / math.sqrt(C1 + C2))
        layer.bias.copy_(rnd(Cout, seed=6) * 0.1)
    x1, x2 = rnd(S, C1, H, H, seed=1), rnd(S, C2, H, H, seed=2)
    ref = F.conv2d(torch.cat([x1, x2], 1).double(), layer.weight.double(), layer.bias.double())
    layer = layer.to(dev)
    with torch.no_grad():
        y = ops.conv1x1_cat(x1.to(dev), x2.to(dev), layer)
    assert rel(y, ref) < 2e-6
    conv = torch.nn.Conv2d(64, 64, 3, padding=1)
    gn = torch.nn.GroupNorm(32, 64)
    with torch.no_grad():
        conv.weight.copy_(rnd(64, 64, 3, 3, seed=7) / 24)
        gn.weight.copy_(1 + 0.2 * rnd(64, seed=8)); gn.bias.copy_(0.2 * rnd(64, seed=9))
    x = rnd(S, 64, 32, 32, seed=3)
    yr = F.conv2d(x.double(), conv.weight.double(), conv.bias.double(), padding=1)
    ar = F.group_norm(yr, 32, gn.weight.double(), gn.bias.double(), eps=1e-5)
    ar = ar * torch.sigmoid(ar)
    conv, gn = conv.to(dev), gn.to(dev)
    with torch.no_grad():
        yg, ag = ops.conv2d_gn(x.to(dev), conv, gn, 32, True, want_y=True)
    assert rel(yg, yr) < 2e-6 and rel(ag, ar) < 1e-5


@pytest.mark.parametrize("Cin,Cout,Hin,mode", [(64, 64, 64, "same"), (6, 64, 64, "same"), (64, 6, 64, "same"),
                                               (192, 64, 64, "same"), (128, 128, 32, "same"), (320, 128, 32, "same"),
                                               (128, 128, 32, "up2"), (192, 192, 16, "up2"), (32, 32, 32, "same"),
                                               (96, 160, 32, "same"), (40, 96, 64, "same"), (192, 192, 16, "same"),
                                               (384, 192, 16, "same"), (128, 128, 8, "up2"), (320, 320, 8, "same"),
                                               (640, 320, 8, "same")])
def test_conv_winograd_path(dev, Cin, Cout, Hin, mode):
    """Fused Winograd F(2x2,3x3) forward, dgrad and (plain stride-1 layers with >= 32 channels) wgrad,
    forced on, vs CPU conv2d."""
    from view_fusion_amd import ops
    ops.st.FORCE_WINOGRAD = True
    try:
        test_conv_fwd_bwd(dev, Cin, Cout, Hin, 3, mode, 3)
    finally:
        ops.st.FORCE_WINOGRAD = False


@pytest.mark.parametrize("Cin,Cout,Hin,mode,S", [
    (64, 64, 64, "same", 3), (6, 64, 64, "same", 3), (64, 6, 64, "same", 3), (192, 64, 64, "same", 2),
    (128, 128, 32, "same", 3), (320, 128, 32, "same", 3), (128, 128, 32, "up2", 2), (192, 192, 16, "up2", 3),
    (96, 160, 32, "same", 5), (40, 96, 64, "same", 2), (13, 70, 32, "same", 7),
    # more than 256 workgroup tiles: persistent workgroups walk on to a second tile (next-tile staging under the epilogue)
    (16, 64, 64, "same", 40), (24, 128, 32, "same", 70),
    # a tail round whose tiles are K-split (partial outputs + fix-up launch) behind a full round
    (128, 128, 32, "same", 80)])
def test_conv_winograd44_path(dev, Cin, Cout, Hin, mode, S):
    """Fused Winograd F(4x4,3x3) forward + dgrad (csrc/winograd44f.hip), forced on wherever the kernel supports the map
    (32x32 / 64x64 outputs), vs CPU conv2d.  rel = max|a - b| / max|b| < 3e-5 (the 4-point transform on both axes:
    measured 4-9e-6; the nested kernel is held to 2e-5)."""
    from view_fusion_amd import ops
    ops.st.FORCE_WINOGRAD44 = True
    try:
        test_conv_fwd_bwd(dev, Cin, Cout, Hin, 3, mode, S, tol=3e-5)
    finally:
        ops.st.FORCE_WINOGRAD44 = False


@pytest.mark.parametrize("Cin,Cout,Hin,mode,S", [(320, 320, 8, "same", 6), (192, 320, 8, "same", 9), (64, 96, 4, "up2", 5),
                                                 (192, 192, 16, "same", 4)])
def test_conv_winograd_small_maps(dev, Cin, Cout, Hin, mode, S):
    """8x8 maps pack four views into one 64-tile workgroup (ragged last group); all tiles K-split."""
    from view_fusion_amd import ops
    ops.st.FORCE_WINOGRAD = True
    try:
        test_conv_fwd_bwd(dev, Cin, Cout, Hin, 3, mode, S)
    finally:
        ops.st.FORCE_WINOGRAD = False


@pytest.mark.parametrize("C,H", [(64, 64), (128, 32), (192, 16), (320, 16), (96, 32), (320, 8), (640, 8), (96, 8)])
def test_group_norm_backward_rowsum(dev, C, H):
    """The GroupNorm backward's closed-form per-(view, channel) sum of dx == the sum of the dx it wrote; a conv
    whose dY is that tensor takes its bias gradients from it (same result as the rowsum kernels)."""
    from view_fusion_amd import ops
    S = 3
    x, gy = rnd(S, C, H, H, seed=1), rnd(S, C, H, H, seed=2)
    gamma, beta = (1 + 0.1 * rnd(C, seed=3)).to(dev), (0.1 * rnd(C, seed=4)).to(dev)
    xg = x.to(dev).requires_grad_(True)
    y = ops.group_norm(xg, gamma, beta, 32, silu=True)
    seen, real_put = [], ops.norm._rowsum_put
    ops.norm._rowsum_put = lambda t, rs, cs: (seen.append((t, rs)), real_put(t, rs, cs))[1]
    try:
        y.backward(gy.to(dev))
    finally:
        ops.norm._rowsum_put = real_put
    (t, rowsum), = seen                           # the dx tensor the kernel wrote, and its closed-form sums
    assert torch.equal(t, xg.grad) and t._vf_sums[0] == t._version and t._vf_sums[1] is rowsum
    ref = t.double().sum((2, 3))
    scale = t.double().abs().sum((2, 3)).max().item()
    assert (rowsum.double() - ref).abs().max().item() < 2e-6 * scale
    # end to end: conv (bias + per-view bias) -> GN -> loss, bias grads with and without the shortcut
    layer = torch.nn.Conv2d(C, C, 3, padding=1).to(dev)
    vb = rnd(S, C, seed=5).to(dev).requires_grad_(True)
    grads = []
    from view_fusion_amd import _lib
    real_call, names = _lib.call, []
    _lib.call = lambda name, *a: (names.append(name), real_call(name, *a))[1]
    try:
        for fusion in (True, False):
            ops.st.ROWSUM_FUSION = fusion
            layer.zero_grad(); vb.grad = None
            del names[:]
            h = ops.conv2d(x.to(dev), layer, view_bias=vb)
            ops.group_norm(h, gamma, beta, 32, silu=True).backward(gy.to(dev))
            grads.append((layer.bias.grad.clone(), vb.grad.clone()))
            # with the sums riding on dY the conv backward re-reads nothing; without them it must
            assert (("vf_rowsum" in names) or ("vf_bias_grad" in names)) == (not fusion), names
    finally:
        _lib.call = real_call
        ops.st.ROWSUM_FUSION = True
    for a, b in zip(*grads):
        assert (a - b).abs().max().item() < 1e-5 * max(1.0, b.abs().max().item()) + 2e-6 * scale


@pytest.mark.parametrize("K,S", [(64, 7), (32, 96)])
def test_time_affine_grouped(dev, K, S):
    """All FeatureWiseAffine linears in one grouped launch == the individual nn.Linear layers (fwd, dW, db, demb)."""
    from view_fusion_amd import ops
    torch.manual_seed(0)
    Cs = [64, 128, 6, 320, 192, 64]
    lin_c = [torch.nn.Linear(K, C) for C in Cs]
    lin_g = [torch.nn.Linear(K, C).to(dev) for C in Cs]
    for a, b in zip(lin_c, lin_g):
        b.load_state_dict(a.state_dict())
    emb = rnd(S, K, seed=1)
    gys = [rnd(S, C, seed=10 + i) for i, C in enumerate(Cs)]
    ec = emb.clone().requires_grad_(True)
    sum((l(ec) * g).sum() for l, g in zip(lin_c, gys)).backward()
    eg = emb.to(dev).requires_grad_(True)
    outs = ops.time_affine_all(eg, lin_g)
    for o, l in zip(outs, lin_c):
        assert rel(o, l(emb)) < 1e-5
    sum((o * g.to(dev)).sum() for o, g in zip(outs, gys)).backward()
    assert rel(eg.grad, ec.grad) < 2e-5
    for a, b in zip(lin_c, lin_g):
        assert rel(b.weight.grad, a.weight.grad) < 2e-5 and rel(b.bias.grad, a.bias.grad) < 2e-5


@pytest.mark.parametrize("C1,C2,H,Cout,S", [(64, 64, 64, 64, 3), (192, 128, 32, 128, 3), (320, 192, 8, 320, 6),
                                             (128, 64, 16, 192, 5), (320, 320, 8, 320, 2)])
def test_cat_free_decoder_ops(dev, C1, C2, H, Cout, S):
    """GroupNorm(+Swish) and the residual 1x1 conv on cat(x1, x2) without building the concatenation:
    forward and every gradient vs the materialised torch reference (groups straddle the split at C = 320)."""
    from view_fusion_amd import ops
    torch.manual_seed(0)
    C = C1 + C2
    x1, x2 = rnd(S, C1, H, H, seed=1), rnd(S, C2, H, H, seed=2)
    gamma, beta = 1 + 0.1 * rnd(C, seed=3), 0.1 * rnd(C, seed=4)
    ga, gr = rnd(S, C, H, H, seed=5), rnd(S, Cout, H, H, seed=6)
    conv_c = torch.nn.Conv2d(C, Cout, 1)
    conv_g = torch.nn.Conv2d(C, Cout, 1).to(dev)
    conv_g.load_state_dict(conv_c.state_dict())
    x1c, x2c, gc, bc = (t.clone().requires_grad_(True) for t in (x1, x2, gamma, beta))
    xc = torch.cat([x1c, x2c], 1)
    ac = F.silu(F.group_norm(xc, 32, gc, bc, 1e-5))
    rc = conv_c(xc)
    ((ac * ga).sum() + (rc * gr).sum()).backward()
    x1g, x2g, gg, bg = (t.to(dev).requires_grad_(True) for t in (x1, x2, gamma, beta))
    assert ops.cat_fusable(C1, C, H * H, 32)
    ag, t1, t2 = ops.group_norm_cat_skip(x1g, x2g, gg, bg, 32, True)
    rg = ops.conv1x1_cat(t1, t2, conv_g)
    assert rel(ag, ac) < 1e-5 and rel(rg, rc) < 2e-5
    ((ag * ga.to(dev)).sum() + (rg * gr.to(dev)).sum()).backward()
    for a, b in ((x1g, x1c), (x2g, x2c), (gg, gc), (bg, bc)):
        assert rel(a.grad, b.grad) < 3e-5
    assert rel(conv_g.weight.grad, conv_c.weight.grad) < 1e-4
    assert rel(conv_g.bias.grad, conv_c.bias.grad) < 2e-5


def test_conv_large_batch_split_k(dev):
    """Stride-1 3x3 layers at large S: S (H/2) (W/2) >= 256 at every shape here, so the weight gradient is the Winograd
    F(4x4) kernel's (vf_wino_wgrad: many chunks per slice; odd S on the 8x8 map, one chunk per view) -- NOT the direct
    kernel's, whose multi-tile slices and two-image 8x8 tiles tests/test_gpu_wgrad_plan.py runs.  The kernel log confirms
    the entry."""
    from view_fusion_amd import ops
    for (Cin, Cout, H, S) in [(64, 64, 64, 40), (320, 320, 8, 97), (192, 192, 16, 96)]:
        layer = torch.nn.Conv2d(Cin, Cout, 3, padding=1)
        x, gy = rnd(S, Cin, H, H, seed=1), rnd(S, Cout, H, H, seed=2)
        xc = x.clone().requires_grad_(True)
        yc = layer(xc); yc.backward(gy)
        wgc = layer.weight.grad.clone(); layer.zero_grad()
        layer = layer.to(dev)
        xg = x.to(dev).requires_grad_(True)
        ops.st.KERNEL_LOG = []
        try:
            yg = ops.conv2d(xg, layer); yg.backward(gy.to(dev))
            torch.cuda.synchronize()
            wgrad = [e[5] for e in ops.st.KERNEL_LOG if e[0] == "conv_wgrad"]
        finally:
            ops.st.KERNEL_LOG = None
        assert wgrad == (["vf_wino_wgrad_main", "vf_wino44_reduce_multi"] if ops.st.WRED_DEFER else ["vf_wino_wgrad"]), wgrad
        assert rel(yg, yc) < 2e-5 and rel(xg.grad, xc.grad) < 2e-5
        assert rel(layer.weight.grad, wgc) < 1e-4


def test_linear_swish_embed(dev):
    from view_fusion_amd import ops
    S, I, O = 7, 64, 256
    x, w, b, gy = rnd(S, I, seed=1), rnd(O, I, seed=2) / 8, rnd(O, seed=3), rnd(S, O, seed=4)
    xc, wc, bc = (t.clone().requires_grad_(True) for t in (x, w, b))
    yc = F.linear(xc, wc, bc); yc = yc * torch.sigmoid(yc); yc.backward(gy)
    xg, wg, bg = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    yg = ops.swish(ops.linear(xg, wg, bg)); yg.backward(gy.to(dev))
    assert rel(yg, yc) < 1e-5
    for a, c in ((xg, xc), (wg, wc), (bg, bc)):
        assert rel(a.grad, c.grad) < 2e-5
    level, angle = torch.rand(S, 1), torch.rand(S, 1) * 6.28
    k = torch.arange(16, dtype=torch.float32) / 16
    enc = lambda v: torch.cat([torch.sin(v * torch.exp(-math.log(1e4) * k)), torch.cos(v * torch.exp(-math.log(1e4) * k))], -1)
    ref = torch.cat([enc(level), enc(angle)], -1)
    got = ops.sincos_embedding(level.to(dev), angle.to(dev), 64)
    assert float((got.cpu() - ref).abs().max()) < 2e-6


@pytest.mark.parametrize("C,H,S", [(192, 16, 3), (320, 8, 3), (64, 8, 3), (192, 16, 56), (96, 16, 53), (64, 16, 1),
                                   (192, 16, 17), (192, 16, 100), (32, 16, 24), (96, 16, 3)])
def test_attention_fwd_bwd(dev, C, H, S):
    """S <= 16 at L=256 (C a multiple of 64) runs the 16-query kernel of round 5 (the sampler's); every other L=256 call the
    32-query kernel (round 5: 8 S workgroups, whole groups of eight views placed per XCD + a plain-order remainder -- S = 17,
    53, 56; C = 32 is its shortest channel loop) or, where 2 S workgroups fill the chip better (S = 100), the 128-query
    kernel.  Both L=64 shapes here (S = 3, C = 320 and 64: multiples of 64) take the 16-query kernel as well -- the L=64
    key-split kernel (S > 16 or C % 64 != 0) runs in tests/test_gpu_attn_plan.py.  All write the probabilities for the backward
    pass here.  Backward at L=256: one launch of the 32-query kernel in its second role (dS from dP = dO^T V and P in registers,
    then dQ = K dS^T) + one launch for dV and dK where C is a multiple of 64 (192, 64), the two batched products otherwise
    (96, 32); at L=64 four batched products + the softmax backward."""
    from view_fusion_amd import ops
    L = H * H
    qkv, gy = rnd(S, 3 * C, H, H, seed=1) * 2, rnd(S, C, H, H, seed=2)
    qc = qkv.clone().requires_grad_(True)
    q, k, v = qc.reshape(S, 3, C, L).unbind(1)
    p = torch.softmax(torch.bmm(q.transpose(1, 2), k) / math.sqrt(C), -1)
    oc = torch.bmm(v, p.transpose(1, 2)).reshape(S, C, H, H)
    oc.backward(gy)
    qg = qkv.to(dev).requires_grad_(True)
    og = ops.attention(qg); og.backward(gy.to(dev))
    assert rel(og, oc) < 2e-5
    assert rel(qg.grad, qc.grad) < 5e-5


@pytest.mark.parametrize("C,H,S", [(192, 16, 2), (320, 8, 2), (32, 32, 2), (192, 16, 12), (192, 16, 40), (192, 16, 60), (320, 8, 40),
                                   (320, 16, 16), (192, 16, 1), (96, 16, 5), (192, 16, 96), (192, 16, 128), (64, 16, 150)])
def test_attention_inference_path(dev, C, H, S):
    """no-grad call: fused kernels without the probability write (L=64: the 16-query kernel at S = 2, the key-split kernel at
    S = 40; L=256: the 16-query kernel up to S = 16 where C is a multiple of 64, the 32-query kernel at S = 5 (C = 96), 40, 60,
    96 and 150, the 128-query kernel at S = 128) / generic path (L=1024)."""
    from view_fusion_amd import ops
    L = H * H
    qkv = rnd(S, 3 * C, H, H, seed=3) * 2
    q, k, v = qkv.reshape(S, 3, C, L).unbind(1)
    p = torch.softmax(torch.bmm(q.transpose(1, 2), k) / math.sqrt(C), -1)
    oc = torch.bmm(v, p.transpose(1, 2)).reshape(S, C, H, H)
    with torch.no_grad():
        og = ops.attention(qkv.to(dev))
    assert rel(og, oc) < 2e-5


def test_concat(dev):
    from view_fusion_amd import ops
    a, b = rnd(3, 64, 8, 8, seed=1), rnd(3, 32, 8, 8, seed=2)
    ag, bg = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    o = ops.concat_channels(ag, bg)
    assert torch.equal(o.cpu(), torch.cat([a, b], 1))
    g = rnd(3, 96, 8, 8, seed=3)
    o.backward(g.to(dev))
    assert torch.equal(ag.grad.cpu(), g[:, :64]) and torch.equal(bg.grad.cpu(), g[:, 64:])


@pytest.mark.parametrize("weighting", [True, False])
def test_compose_loss_and_stack(dev, weighting):
    from oracle import view_fusion_ref as vfr
    from view_fusion_amd import ops
    B, N, H = 4, 5, 16
    vc = [1, 5, 3, 2]
    g = torch.Generator().manual_seed(3)
    y_cond, y_0 = torch.rand(B, N, 3, H, H, generator=g), torch.rand(B, 3, H, H, generator=g)
    noise, level, angle = torch.randn(B, 3, H, H, generator=g), torch.rand(B, generator=g), torch.rand(B, 1, generator=g)
    off, S, maxv = ops.view_offsets(vc, dev)
    assert (S, maxv) == (11, 5)
    x, ls, as_ = ops.stack_views(y_cond.to(dev), y_0.to(dev), noise.to(dev), level.to(dev), angle.to(dev), off, S)
    yn = vfr.q_sample(y_0, level.reshape(-1, 1, 1, 1), noise)
    xr, ar, lr = vfr.stack_views(y_cond, vc, yn, level.reshape(-1, 1), angle)
    assert rel(x, xr) < 1e-6 and torch.equal(ls.cpu(), lr) and torch.equal(as_.cpu(), ar)

    out = torch.randn(S, 6, H, H, generator=g) * 2
    oc = out.clone().requires_grad_(True)
    nh, _, w = vfr.compose(oc, vc, weighting)
    lc = F.mse_loss(noise, nh); (lc * 1.7).backward()
    og = out.to(dev).requires_grad_(True)
    lg = ops.compose_mse_loss(og, noise.to(dev), off, B, weighting); (lg * 1.7).backward()
    assert abs(lg.item() - lc.item()) < 1e-6 * abs(lc.item()) + 1e-7
    assert rel(og.grad, oc.grad) < 1e-5
    nh2, w2 = ops.compose(out.to(dev), off, B, maxv, weighting)
    assert rel(nh2, nh) < 1e-5
    if weighting:
        assert rel(w2, w) < 1e-5
    else:
        assert w2 is None


def test_p_sample_tail(dev):
    from oracle import view_fusion_ref as vfr
    from view_fusion_amd import ops
    B, H, vc = 3, 16, [2, 1, 3]
    sched = vfr.schedule_buffers(vfr.beta_schedule("linear", 1000, 1e-4, 0.09))
    g = torch.Generator().manual_seed(5)
    out, y_t, z = torch.randn(6, 6, H, H, generator=g), torch.randn(B, 3, H, H, generator=g), torch.randn(B, 3, H, H, generator=g)
    t = torch.tensor([999, 400, 1])
    eps, _, w = vfr.compose(out, vc, True)
    pick = lambda k: sched[k][t].reshape(-1, 1, 1, 1)
    y0 = (pick("sqrt_recip_gammas") * y_t - pick("sqrt_recipm1_gammas") * eps).clamp(-1, 1)
    mean = pick("posterior_mean_coef1") * y0 + pick("posterior_mean_coef2") * y_t
    ref = mean + z * (0.5 * pick("posterior_log_variance_clipped")).exp()
    off, S, maxv = ops.view_offsets(vc, dev)
    sd = {k: v.to(dev) for k, v in sched.items()}
    y, m, w2 = ops.p_sample_tail(out.to(dev), off, y_t.to(dev), z.to(dev), t.to(dev), sd, B, maxv, True, want_mean=True)
    assert rel(y, ref) < 1e-5 and rel(m, mean) < 1e-5 and rel(w2, w) < 1e-5


def test_fused_adam_matches_torch_adam(dev):
    from view_fusion_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(0)
    shapes = [(64, 6, 3, 3), (6,), (320, 320, 3, 3), (1027,), (64, 64)]
    pc = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    pg = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in pc]
    oc, og = torch.optim.Adam(pc, lr=1e-3), FusedAdam(pg, lr=1e-3)
    for it in range(4):
        for a, b in zip(pc, pg):
            gr = torch.randn(a.shape, generator=g)
            a.grad, b.grad = gr.clone(), gr.to(dev)
        lr = 1e-3 * (it + 1)
        for o in (oc, og):
            o.param_groups[0]["lr"] = lr
            o.step()
    for a, b in zip(pc, pg):
        assert rel(b, a) < 1e-6
    sd = og.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 4


# ------------------------------------------------------------------------------------------------
# Round 3: the Winograd F(4x4,3x3) weight-gradient kernel and the bf16x3 1x1 experiment, through the C ABI directly
def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("Cin,Cout,H,mode,S", [(64, 64, 64, 0, 5), (6, 64, 64, 0, 3), (64, 6, 32, 0, 7), (96, 160, 32, 0, 4),
                                               (128, 192, 16, 0, 9), (320, 320, 8, 0, 7), (192, 64, 8, 0, 1),
                                               (128, 128, 32, 2, 3), (192, 192, 16, 2, 5), (320, 128, 8, 2, 6)])
def test_wino44_wgrad_vs_fp64(dev, Cin, Cout, H, mode, S):
    """vf_wino_wgrad (Winograd F(4x4,3x3), K split over workgroups + slab sum) against an fp64 correlation on the CPU:
    dW rel-L2 <= 2e-5 (measured 2-5e-6; the direct fp32 kernel 3e-6), bias gradient and its second copy <= 1e-5.
    Covers clamped channel tiles (Cin / Cout = 6), odd view counts on 8x8 maps (one chunk per view), uneven K slices
    and the upsampled-input mode."""
    from view_fusion_amd import _lib, ops
    lib = _lib.load()
    Hx = H // 2 if mode == 2 else H
    x = rnd(S, Cin, Hx, Hx, seed=21)
    dy = rnd(S, Cout, H, H, seed=22)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if mode == 2 else x
    xp = F.pad(xin.double(), (1, 1, 1, 1))
    ref = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64)
    for p in range(3):
        for q in range(3):
            ref[:, :, p, q] = torch.einsum("sohw,sihw->oi", dy.double(), xp[:, :, p:p + H, q:q + H])
    xg, dyg = x.to(dev), dy.to(dev)
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), device=dev)
    db = torch.full((Cout,), float("nan"), device=dev)
    db2 = torch.full((Cout,), float("nan"), device=dev)
    ws = torch.empty(lib.vf_wino_wgrad_ws_floats(S, Cin, Cout, H, H), device=dev)
    _lib.call("vf_wino_wgrad", xg.data_ptr(), dyg.data_ptr(), dw.data_ptr(), db.data_ptr(), db2.data_ptr(), ws.data_ptr(),
              ws.numel(), S, Cin, Cout, H, H, mode, ops._stream())
    torch.cuda.synchronize()
    assert _rel_l2(dw, ref) < 2e-5
    dbr = dy.double().sum(dim=(0, 2, 3))
    assert _rel_l2(db, dbr) < 1e-5 and torch.equal(db, db2)


def test_wino44_wgrad_is_deterministic(dev):
    """Two launches on the same inputs give bit-identical results (fixed summation order, no float atomics)."""
    from view_fusion_amd import _lib, ops
    lib = _lib.load()
    S, Cin, Cout, H = 24, 128, 64, 32
    x, dy = rnd(S, Cin, H, H, seed=31).to(dev), rnd(S, Cout, H, H, seed=32).to(dev)
    ws = torch.empty(lib.vf_wino_wgrad_ws_floats(S, Cin, Cout, H, H), device=dev)
    outs = []
    for _ in range(2):
        dw = torch.empty(Cout, Cin, 3, 3, device=dev)
        _lib.call("vf_wino_wgrad", x.data_ptr(), dy.data_ptr(), dw.data_ptr(), None, None, ws.data_ptr(), ws.numel(), S, Cin,
                  Cout, H, H, 0, ops._stream())
        outs.append(dw.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("Cin,Cout,H,S,cat_in,cat_out", [(192, 576, 16, 3, 0, 0), (64, 6, 64, 2, 0, 0), (96, 200, 8, 3, 0, 0),
                                                         (320, 128, 32, 2, 128, 0), (128, 320, 32, 2, 0, 192),
                                                         (640, 320, 8, 5, 320, 0)])
def test_conv1x1_bf16x3_vs_fp64(dev, Cin, Cout, H, S, cat_in, cat_out):
    """The bf16x3 split-product 1x1 convolution (experiment, default off) is fp32-ACCURATE: rel-L2 error against fp64
    <= 1e-6 (measured 1-5e-7, below the fp32-MFMA kernel's).  Covers bias + per-view bias + residual, channel tiles
    beyond Cout, a column count that is no multiple of the 128-column tile, the concatenated input and the split output."""
    from view_fusion_amd import _lib, ops
    lib = _lib.load()
    st = ops._stream()
    w = rnd(Cout, Cin, seed=41) / math.sqrt(Cin)
    x = rnd(S, Cin, H, H, seed=42)
    bias, vb, res = rnd(Cout, seed=43), rnd(S, Cout, seed=44), rnd(S, Cout, H, H, seed=45)
    use_epi = not cat_out
    ref = torch.einsum("oi,sihw->sohw", w.double(), x.double())
    if use_epi:
        ref = ref + bias.double()[None, :, None, None] + vb.double()[:, :, None, None] + res.double()
    wg = w.to(dev).contiguous()
    w3 = torch.empty(lib.vf_conv1x1_bf16x3_pack_dwords(Cout, Cin), device=dev, dtype=torch.int32)
    _lib.call("vf_conv1x1_bf16x3_pack", wg.data_ptr(), w3.data_ptr(), None, Cout, Cin, st)
    if cat_in:
        x1, x2 = x[:, :cat_in].contiguous().to(dev), x[:, cat_in:].contiguous().to(dev)
    else:
        x1, x2 = x.to(dev), None
    if cat_out:
        y1 = torch.full((S, cat_out, H, H), float("nan"), device=dev)
        y2 = torch.full((S, Cout - cat_out, H, H), float("nan"), device=dev)
    else:
        y1, y2 = torch.full((S, Cout, H, H), float("nan"), device=dev), None
    P = lambda t: t.data_ptr() if t is not None else None
    bg, vg, rg = (bias.to(dev), vb.to(dev), res.to(dev)) if use_epi else (None, None, None)   # (kept alive across the call)
    _lib.call("vf_conv1x1_bf16x3", P(x1), P(x2), cat_in, w3.data_ptr(), P(bg), P(vg), P(rg), P(y1), P(y2), cat_out, S, Cin,
              Cout, H * H, st)
    torch.cuda.synchronize()
    y = torch.cat((y1, y2), dim=1) if cat_out else y1
    assert _rel_l2(y, ref) < 1e-6
