"""LPIPS (vgg, version 0.1), the reference's third eval metric (utils/compute_metrics.py:
lpips.LPIPS(net="vgg")(2 * gen - 1, 2 * target - 1)) on the engine's own kernels: the thirteen 3x3 convolutions of the
VGG16 trunk through ops.conv2d, everything around them in csrc/lpips.hip.  Inference only, no backward."""
import torch

from .. import _lib
from .conv import conv2d
from .core import _c, _call, _check, _ptr, _stream

LPIPS_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)   # the 13 convs of VGG16 `features`
LPIPS_TAPS = (1, 3, 6, 9, 12)              # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3: the conv that ends each group
LPIPS_MIN_SIDE, LPIPS_SIDE_MULTIPLE = 32, 16


def _conv(x, layer):
    try:
        return conv2d(x, layer)
    except _lib.VFHipError as exc:
        if not str(exc).endswith("hipError_t 1"):       # anything but "invalid value" is not a refused geometry
            raise
        raise ValueError(f"lpips: ops.conv2d refuses a {layer.weight.shape[1]} -> {layer.weight.shape[0]} channel 3x3 "
                         f"convolution on {x.shape[0]} maps of {x.shape[2]}x{x.shape[3]} (vf_conv_fwd: 3x3 'same' "
                         f"layers need a non-empty map of at most 2^30 stacked pixels)") from exc


def lpips(generated, target, net):
    """Per-pair LPIPS (B,) float32 of two (B,3,H,W) tensors in [0,1].  `net`: a drivers.LPIPS (`.convs`: the 13 conv
    holders, `.lins`: the five (1,C,1,1) lin weights).  H and W must be multiples of 16 and at least 32 (the five tap
    maps are H x W ... H/16 x W/16).  Both images go through the trunk as one stacked batch of 2B."""
    if generated.dim() != 4 or generated.shape != target.shape or generated.shape[1] != 3:
        raise ValueError(f"lpips needs two (B,3,H,W) tensors of one shape, got {tuple(generated.shape)} and "
                         f"{tuple(target.shape)}")
    B, _, H, W = generated.shape
    if H % LPIPS_SIDE_MULTIPLE or W % LPIPS_SIDE_MULTIPLE or H < LPIPS_MIN_SIDE or W < LPIPS_MIN_SIDE:
        raise ValueError(f"lpips needs H and W to be multiples of {LPIPS_SIDE_MULTIPLE} and at least {LPIPS_MIN_SIDE} "
                         f"(smaller images lose a tap map), got {tuple(generated.shape)}")
    generated, target = _c(generated), _c(target)
    _check(generated, target)
    dev = generated.device
    out = torch.empty(B, device=dev, dtype=torch.float32)
    if B == 0:
        return out
    lib = _lib.load()
    tiles = [lib.vf_lpips_layer_tiles(LPIPS_WIDTHS[i], (H >> l) * (W >> l)) for l, i in enumerate(LPIPS_TAPS)]
    slots = sum(tiles)
    assert B * slots == lib.vf_lpips_workspace_floats(B, H, W)
    S = 2 * B
    with torch.no_grad():
        # (a buffer of its own: the convs between two taps use the shared split-K workspace)
        ws = torch.empty(B * slots, device=dev, dtype=torch.float32)
        x = torch.empty(S, 3, H, W, device=dev, dtype=torch.float32)
        _call("vf_lpips_prep", _ptr(generated), _ptr(target), _ptr(x), B, H * W, _stream())
        tap, slot0 = 0, 0
        for i, layer in enumerate(net.convs):
            y = _conv(x, layer)
            _, C, h, w = y.shape
            if i != LPIPS_TAPS[tap]:
                _call("vf_relu", _ptr(y), y.numel(), _stream())
                x = y
                continue
            if tap < 4:          # the tap and the next group's input from one read of the conv output
                x = torch.empty(S, C, h // 2, w // 2, device=dev, dtype=torch.float32)
                _call("vf_relu_maxpool2", _ptr(y), _ptr(x), S * C, h, w, _stream())
            else:
                _call("vf_relu", _ptr(y), y.numel(), _stream())
            lin = net.lins[tap]
            _check(lin)
            if lin.numel() != C:
                raise ValueError(f"lpips: lin{tap} has {lin.numel()} weights for a tap of {C} channels")
            _call("vf_lpips_layer", _ptr(y), _ptr(lin), _ptr(ws), B, C, h * w, slot0, slots, _stream())
            slot0 += tiles[tap]
            tap += 1
        _call("vf_lpips_finish", _ptr(ws), _ptr(out), B, slots, _stream())
    return out
