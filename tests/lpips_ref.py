"""Test infrastructure: two independent restatements of lpips.LPIPS(net="vgg", version "0.1")(2 x - 1, 2 y - 1) for
images in [0, 1], the synthetic network and the table of inputs the LPIPS tests share.  Neither the lpips package nor
torchvision is a dependency of this repository, so nothing is pinned to them; the product never imports this file.

    lpips_fp32   torch-CPU fp32 in the package's operation order: ScalingLayer, the VGG16 `features` slices with
                 F.conv2d / relu / max_pool2d, normalize_tensor (x / (sqrt(sum x^2) + 1e-10)), the squared difference,
                 the 1x1 lin convolution, the spatial mean, the sum over the five taps.
    lpips_fp64   numpy float64, written separately: every 3x3 convolution is an im2col gather and a matrix product,
                 the pool a reshape, the distance an einsum.  The truth.

A network is the pair (vgg_sd, lin_sd) of state dicts in the formats drivers.LPIPS.from_state_dicts accepts.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10
CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)     # torchvision's vgg16().features
WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
GROUPS = (2, 2, 3, 3, 3)                                          # convs per group; the tap is the group's last ReLU
TAP_C = (64, 128, 256, 512, 512)
KINDS = ["noisy", "unrelated", "identical", "flat"]


def make_net(seed, dead_tail=False):
    """The real VGG16 widths with seeded weights: conv N(0, 2 / fan_in), biases small and of both signs, lin uniform in
    [0, 1/C] (non-negative, as the shipped ones).  dead_tail: the biases of the last group are -10, so relu5_3 is all
    zero for every input and the whole tap sits on the 1e-10 epsilon."""
    g = torch.Generator().manual_seed(seed)
    vgg, cin = {}, 3
    for n, (idx, cout) in enumerate(zip(CONV_IDX, WIDTHS)):
        vgg[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
        vgg[f"features.{idx}.bias"] = (torch.rand(cout, generator=g) - 0.5) * 0.2
        if dead_tail and n >= 10:
            vgg[f"features.{idx}.bias"] = torch.full((cout,), -10.0)
        cin = cout
    lin = {f"lin{l}.model.1.weight": torch.rand(1, C, 1, 1, generator=g) / C for l, C in enumerate(TAP_C)}
    return vgg, lin


def only_tap(net, tap):
    """The same network with every lin weight zero except tap `tap`'s."""
    vgg, lin = net
    return vgg, {k: (v if k == f"lin{tap}.model.1.weight" else torch.zeros_like(v)) for k, v in lin.items()}


def make_pair(kind, B, H, W, seed=0):
    """One (generated, target) pair of float32 CPU (B,3,H,W) tensors in [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.arange(H, dtype=torch.float32).reshape(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float32).reshape(1, 1, 1, W)
    ph = torch.rand(B, 3, 1, 1, generator=g) * 6.2831853
    base = (0.5 + 0.4 * torch.sin(0.23 * xx + ph) * torch.cos(0.17 * yy + 0.5 * ph)).contiguous()
    if kind == "noisy":
        return (base + 0.05 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1), base
    if kind == "unrelated":
        return torch.rand(B, 3, H, W, generator=g), base
    if kind == "identical":
        return base, base.clone()
    if kind == "flat":
        c = torch.rand(2, B, 3, 1, 1, generator=g)
        return c[0].expand(B, 3, H, W).contiguous(), c[1].expand(B, 3, H, W).contiguous()
    raise ValueError(kind)


# ---- fp32, the package's order -----------------------------------------------------------------------------------
def distance_fp32(feats_a, feats_b, lins):
    """sum over taps of spatial_average(lin(normalize(a) - normalize(b))^2): lists of (B,C,h,w) and of (1,C,1,1)."""
    val = 0
    for a, b, w in zip(feats_a, feats_b, lins):
        na = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + EPS)
        nb = b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + EPS)
        val = val + F.conv2d((na - nb) ** 2, w).mean([2, 3], keepdim=True)
    return val.reshape(-1)


def _taps_fp32(x, vgg):
    shift = torch.tensor(SHIFT).reshape(1, 3, 1, 1)
    scale = torch.tensor(SCALE).reshape(1, 3, 1, 1)
    h = (2 * x - 1 - shift) / scale
    taps, it = [], iter(CONV_IDX)
    for gi, n in enumerate(GROUPS):
        if gi:
            h = F.max_pool2d(h, kernel_size=2, stride=2)
        for _ in range(n):
            i = next(it)
            h = F.relu(F.conv2d(h, vgg[f"features.{i}.weight"], vgg[f"features.{i}.bias"], padding=1))
        taps.append(h)
    return taps


def lpips_fp32(generated, target, net):
    """(B,3,H,W) float32 CPU tensors in [0,1] -> (B,) float32."""
    vgg, lin = net
    with torch.no_grad():
        fa, fb = _taps_fp32(generated.float(), vgg), _taps_fp32(target.float(), vgg)
        return distance_fp32(fa, fb, [lin[f"lin{l}.model.1.weight"] for l in range(5)])


# ---- fp64, numpy ---------------------------------------------------------------------------------------------------
def distance_fp64(feats_a, feats_b, lins):
    """Lists of (B,C,h,w) float64 arrays and of (C,) float64 weights -> (B,) float64."""
    total = 0.0
    for a, b, w in zip(feats_a, feats_b, lins):
        ha = a / (np.sqrt(np.einsum("bchw,bchw->bhw", a, a))[:, None] + EPS)
        hb = b / (np.sqrt(np.einsum("bchw,bchw->bhw", b, b))[:, None] + EPS)
        d = np.einsum("c,bchw->bhw", np.asarray(w, dtype=np.float64).reshape(-1), (ha - hb) ** 2)
        total = total + d.reshape(d.shape[0], -1).sum(axis=1) / (d.shape[1] * d.shape[2])
    return total


def _conv3x3_fp64(x, w, b):
    """x (B,Cin,H,W), w (Cout,Cin,3,3), b (Cout,): zero padding 1, as an im2col gather and one matrix product."""
    B, Cin, H, W = x.shape
    xp = np.zeros((B, Cin, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    cols = np.empty((B, H * W, Cin * 9))
    for kh in range(3):
        for kw in range(3):
            cols[:, :, kh * 3 + kw::9] = xp[:, :, kh:kh + H, kw:kw + W].reshape(B, Cin, H * W).transpose(0, 2, 1)
    y = cols @ w.reshape(w.shape[0], Cin * 9).T + b
    return y.transpose(0, 2, 1).reshape(B, w.shape[0], H, W)


def _taps_fp64(x, vgg):
    h = (2.0 * x - 1.0 - np.array(SHIFT).reshape(1, 3, 1, 1)) / np.array(SCALE).reshape(1, 3, 1, 1)
    taps, it = [], iter(CONV_IDX)
    for gi, n in enumerate(GROUPS):
        if gi:
            B, C, H, W = h.shape
            h = h.reshape(B, C, H // 2, 2, W // 2, 2).max(axis=(3, 5))
        for _ in range(n):
            i = next(it)
            h = np.maximum(_conv3x3_fp64(h, vgg[f"features.{i}.weight"].double().numpy(),
                                         vgg[f"features.{i}.bias"].double().numpy()), 0.0)
        taps.append(h)
    return taps


def lpips_fp64(generated, target, net):
    """(B,3,H,W) tensors -> (B,) float64 numpy array."""
    vgg, lin = net
    x = generated.detach().cpu().double().numpy()
    y = target.detach().cpu().double().numpy()
    return distance_fp64(_taps_fp64(x, vgg), _taps_fp64(y, vgg),
                         [lin[f"lin{l}.model.1.weight"].double().numpy() for l in range(5)])


def bound(generated, target, net):
    """The per-case tolerance of the GPU tests: r64 = lpips_fp64, e = max |lpips_fp32 - r64| on these very inputs, and
    per image max(4 e, 1e-4 |r64| + 1e-6) on |gpu - r64|: 4 e for another equally legitimate fp32 summation order (the
    SSIM tests' rule), 1e-4 relative the engine's stated forward tolerance for a deeper stack of the same conv kernels,
    Winograd routes included, 1e-6 the floor for values near zero.  Returns (r64, e, bound (B,))."""
    r64 = lpips_fp64(generated, target, net)
    e = float(np.abs(lpips_fp32(generated, target, net).double().numpy() - r64).max())
    return r64, e, np.maximum(4.0 * e, 1e-4 * np.abs(r64) + 1e-6)


@functools.lru_cache(maxsize=None)
def net_cached(seed=0, dead_tail=False):
    return make_net(seed, dead_tail)


@functools.lru_cache(maxsize=None)
def case(kind, B, H, W, seed=0, tap=None, dead_tail=False):
    """(generated, target, net, r64, e, bound) of a shared, seeded case: computed once, never modified."""
    net = net_cached(0, dead_tail)
    if tap is not None:
        net = only_tap(net, tap)
    X, Y = make_pair(kind, B, H, W, seed)
    return (X, Y, net) + bound(X, Y, net)
