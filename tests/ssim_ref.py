"""Test infrastructure: two independent restatements of pytorch_msssim.ssim(X, Y, data_range, size_average=False)
with the package's defaults (11-tap Gaussian, sigma 1.5, "valid" separable filtering, K = (0.01, 0.03), no clamp), and
the table of inputs the SSIM tests share.  The package itself is not a dependency of this repository, so nothing is
pinned to it; the product never imports this file.

    ssim_fp32   torch-CPU fp32, the package's operation order restated literally (grouped conv2d along H, then along
                W, the five maps, the two ratios, the mean per channel and then over channels): what the reference
                would compute.
    ssim_fp64   numpy float64 with scipy.ndimage.correlate1d, cropped to the valid region: the truth.
"""
import numpy as np
import torch
import torch.nn.functional as F
from scipy.ndimage import correlate1d

WIN, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03

SIZES = [(64, 64), (48, 64), (11, 11), (24, 40), (128, 128), (256, 256), (12, 200)]
CLASSES = ["rand_rand", "noisy", "ident", "const", "flat_noise"]


def window_fp32():
    coords = torch.arange(WIN, dtype=torch.float32)
    coords -= WIN // 2
    g = torch.exp(-(coords ** 2) / (2 * SIGMA ** 2))
    g /= g.sum()
    return g


def ssim_fp32(X, Y, data_range=1.0):
    """(B,C,H,W) float32 CPU tensors -> (B,) float32."""
    X, Y = X.float(), Y.float()
    C = X.shape[1]
    win = window_fp32().reshape(1, 1, 1, WIN).repeat(C, 1, 1, 1)

    def filt(t):
        out = t
        for i, s in enumerate(t.shape[2:]):
            assert s >= WIN
            out = F.conv2d(out, weight=win.transpose(2 + i, -1), stride=1, padding=0, groups=C)
        return out

    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    mu1, mu2 = filt(X), filt(Y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = filt(X * X) - mu1_sq
    sigma2_sq = filt(Y * Y) - mu2_sq
    sigma12 = filt(X * Y) - mu1_mu2
    cs_map = (2 * sigma12 + C2) / (sigma1_sq + sigma2_sq + C2)
    ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return torch.flatten(ssim_map, 2).mean(-1).mean(1)


def ssim_fp64(X, Y, data_range=1.0):
    """(B,C,H,W) tensors / arrays -> (B,) float64 numpy array."""
    x = np.asarray(X.detach().cpu() if torch.is_tensor(X) else X, dtype=np.float64)
    y = np.asarray(Y.detach().cpu() if torch.is_tensor(Y) else Y, dtype=np.float64)
    k = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-(k ** 2) / (2 * SIGMA ** 2))
    g /= g.sum()
    h = WIN // 2

    def filt(a):
        a = correlate1d(correlate1d(a, g, axis=2, mode="constant"), g, axis=3, mode="constant")
        return a[:, :, h:a.shape[2] - h, h:a.shape[3] - h]

    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    mx, my = filt(x), filt(y)
    sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    m = ((2 * mx * my + C1) / (mx * mx + my * my + C1)) * ((2 * sxy + C2) / (sxx + syy + C2))
    return m.reshape(m.shape[0], -1).mean(axis=1)


def make_pair(kind, B, C, H, W, seed=0):
    """One (generated, target) pair of float32 CPU tensors in [0, 1] of input class `kind`."""
    g = torch.Generator().manual_seed(seed)
    if kind == "rand_rand":
        return torch.rand(B, C, H, W, generator=g), torch.rand(B, C, H, W, generator=g)
    if kind == "noisy":
        yy = torch.arange(H, dtype=torch.float32).reshape(1, 1, H, 1)
        xx = torch.arange(W, dtype=torch.float32).reshape(1, 1, 1, W)
        ph = torch.rand(B, C, 1, 1, generator=g) * 6.2831853
        base = 0.5 + 0.4 * torch.sin(0.11 * xx + ph) * torch.cos(0.07 * yy + 0.5 * ph)
        return (base + 0.05 * torch.randn(B, C, H, W, generator=g)).clamp(0, 1), base
    if kind == "ident":
        a = torch.rand(B, C, H, W, generator=g)
        return a, a.clone()
    if kind == "const":
        return torch.full((B, C, H, W), 0.25), torch.full((B, C, H, W), 0.75)
    if kind == "flat_noise":
        return torch.full((B, C, H, W), 0.9), 0.9 + 0.002 * torch.randn(B, C, H, W, generator=g)
    raise ValueError(kind)


def bound(X, Y, data_range=1.0):
    """The per-case tolerance of the GPU tests: e = max |ssim_fp32 - ssim_fp64| on these very inputs, and the bound
    max(4 e, 1e-6) on |gpu - ssim_fp64| (4 x for another equally legitimate fp32 summation order: fma contraction,
    tap order, tile-partial order; the floor for e = 0).  Returns (ssim_fp64, e, bound)."""
    r64 = ssim_fp64(X, Y, data_range)
    e = float(np.abs(ssim_fp32(X, Y, data_range).double().numpy() - r64).max())
    return r64, e, max(4.0 * e, 1e-6)
