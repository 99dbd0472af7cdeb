"""The ViewFusion ops around the UNet: view stacking + q_sample, compose / weighted-noise loss, the sampler tail, PSNR
and SSIM (reference model/view_fusion.py:70-177, 229-300; utils/metrics.py:6-12)."""
import ctypes
import math
import struct

import torch

from .. import _lib
from ..schedule import check_prediction
from .state import st
from .core import _c, _call, _check, _ptr, _stream, _workspace


# ---------------------------------------------------------------------------------------------
# ViewFusion glue


def view_offsets(view_count, device):
    """view_count (list / CPU tensor / device tensor) -> (off int32 [B+1] on device, S, maxV).

    A CPU-side view_count (what the harness and INTEGRATION.md hand over) needs no device sync.  A DEVICE tensor
    (what the reference's loops produce with `.to(device)`, experiment.py:277-279, 476-478) must be read back once,
    because S sizes every allocation -- the same one D2H the reference pays in `cumsum(view_count).tolist()`
    (view_fusion.py:95, 244); the result is remembered per tensor object and version, so a caller that drives
    `p_sample` / `p_mean_variance` step by step with the same device tensor syncs once, not once per step
    (`generate` resolves it once per call anyway).
    """
    if torch.is_tensor(view_count) and view_count.is_cuda:
        for ent in st._VC_CACHE:
            if ent[0] is view_count and ent[1] == view_count._version and ent[2][0].device == device:
                return ent[2]
        vc = view_count.detach().cpu().tolist()
    elif torch.is_tensor(view_count):
        vc = view_count.detach().tolist()
    else:
        vc = [int(v) for v in view_count]
    off = [0]
    for v in vc:
        if v < 1:
            raise ValueError("every sample needs at least one conditioning view")
        off.append(off[-1] + int(v))
    t = torch.tensor(off, dtype=torch.int32)
    if device.type == "cuda":
        t = t.pin_memory().to(device, non_blocking=True)
    out = (t, off[-1], max(vc))
    if torch.is_tensor(view_count) and view_count.is_cuda:
        st._VC_CACHE.insert(0, (view_count, view_count._version, out))
        del st._VC_CACHE[4:]
    return out


def gather_level(gammas, t, u=None):
    """level[b] = gammas[t[b]]  or the training draw (g[t]-g[t-1])*u + g[t-1]."""
    _check(gammas, u)
    t = _c(t.to(torch.int64))
    B = t.numel()
    level = torch.empty(B, device=gammas.device, dtype=torch.float32)
    _call("vf_gather_level", _ptr(gammas), ctypes.c_void_p(t.data_ptr()), _ptr(u), _ptr(level), B, _stream())
    return level


# ---- seeded draws (csrc/rng.h): pure functions of (seed, sample id, kind, step, element) ----
RNG_TRAIN_NOISE, RNG_START_NOISE, RNG_STEP_NOISE = 1, 2, 3        # kinds (0 = the training scalars of draw_train)


def _seed(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def sample_ids(device, B, ids=None):
    """The per-sample identifiers of the seeded draws as a contiguous device int64 (B,): `ids` (tensor / list) when
    given, else arange(B), kept per (device, B).  A host-side `ids` is copied to the device here, so hand a device
    tensor to anything that is captured into a graph."""
    if ids is None:
        ids = st._RNG_IDS.get((device, B))
        if ids is None:
            ids = st._RNG_IDS[(device, B)] = torch.arange(B, dtype=torch.int64, device=device)
        return ids
    ids = torch.as_tensor(ids).reshape(-1)
    if ids.numel() != B:
        raise ValueError(f"sample_ids needs one id per sample: {ids.numel()} ids for a batch of {B}")
    return _c(ids.to(device=device, dtype=torch.int64))


def _check_ids(ids, B):
    if not ids.is_cuda or ids.dtype != torch.int64 or not ids.is_contiguous() or ids.numel() != B:
        raise _lib.VFHipError(f"ids must be a contiguous device int64 tensor of {B} elements (ops.sample_ids)")


def draw_train(seed, ids, gammas, want_u=False):
    """The training scalars of samples `ids`: -> t (B,) int64 in [1, T-1], level (B,) = (g[t]-g[t-1]) u + g[t-1],
    u (B,) in [0, 1) | None.  One launch; replaces randint + rand + gather_level."""
    _check(gammas)
    B = ids.numel()
    _check_ids(ids, B)
    t = torch.empty(B, device=gammas.device, dtype=torch.int64)
    level = torch.empty(B, device=gammas.device, dtype=torch.float32)
    u = torch.empty(B, device=gammas.device, dtype=torch.float32) if want_u else None
    _call("vf_draw_train", _seed(seed), ctypes.c_void_p(ids.data_ptr()), _ptr(gammas), gammas.numel(),
          ctypes.c_void_p(t.data_ptr()), _ptr(u), _ptr(level), B, _stream())
    return t, level, u


def randn_ids(seed, ids, kind, step, shape, out=None):
    """Standard normals (B, *shape) for samples `ids`: element e of a sample is normal e % 4 of float4 block e // 4."""
    B = ids.numel()
    _check_ids(ids, B)
    n = 1
    for d in shape:
        n *= int(d)
    if out is None:
        out = torch.empty(B, *shape, device=ids.device, dtype=torch.float32)
    _check(out)
    _call("vf_randn_ids", _seed(seed), ctypes.c_void_p(ids.data_ptr()), int(kind), int(step), _ptr(out), B, n,
          _stream())
    return out


def philox_ids(seed, ids, kind, step, n):
    """The raw 32-bit words behind randn_ids (as int32 bit patterns, (B, n)): tests compare them with the host."""
    B = ids.numel()
    _check_ids(ids, B)
    out = torch.empty(B, n, device=ids.device, dtype=torch.int32)
    _call("vf_philox_ids", _seed(seed), ctypes.c_void_p(ids.data_ptr()), int(kind), int(step),
          ctypes.c_void_p(out.data_ptr()), B, n, _stream())
    return out


def stack_views(y_cond, y_t, noise, level, angle, off, S, x=None, copy_cond=True, drop=None, null_rows=False,
                self_cond=None, sc_channels=False):
    """Ragged stacking (+ optional q_sample): -> x (S,Cc+3,H,W), level_s (S,1), angle_s (S,1); Cc = y_cond's
    channel count (3, or 6 for the `relative` configs).
    Classifier-free guidance (csrc/diffusion.hip), through a sibling kernel taken only when one of the two is used:
    drop (device bool / uint8 (B,)): the conditioning half of every row of a sample with drop[b] != 0 is zeros;
    null_rows=True: S + B rows come back, row S + b = [ 0 | y_t[b] ] with the sample's own level and angle.
    Self-conditioning (csrc/diffusion.hip), the guided kernel's SC instantiation, taken only when asked for: self_cond (B,3,H,W) --
    x is (rows,Cc+6,H,W) and every row of sample b (its null row too) ends with self_cond[b]; sc_channels=True with
    self_cond=None writes zeros there ("no estimate").  The first Cc + 3 channels carry the bits of the call without it."""
    y_cond, y_t = _c(y_cond), _c(y_t)
    angle = _c(angle.reshape(-1).float())
    _check(y_cond, y_t, noise, level, angle)
    B, Nmax, Cc, H, W = y_cond.shape
    if y_t.shape[1] != 3:
        raise ValueError(f"the noisy target must have 3 channels, got {tuple(y_t.shape)}")
    rows = S + B if null_rows else S
    sc_on = self_cond is not None or sc_channels
    Cx = Cc + (6 if sc_on else 3)
    if x is None:
        x = torch.empty(rows, Cx, H, W, device=y_cond.device, dtype=torch.float32)
    elif x.shape[0] != rows:
        raise ValueError(f"stack_views writes {rows} rows, x has {x.shape[0]}")
    ls = torch.empty(rows, 1, device=y_cond.device, dtype=torch.float32)
    as_ = torch.empty(rows, 1, device=y_cond.device, dtype=torch.float32)
    if sc_on:
        _check(x, self_cond)
        if tuple(x.shape) != (rows, Cx, H, W):
            raise ValueError(f"a self-conditioned stack_views writes x of shape {(rows, Cx, H, W)}, got {tuple(x.shape)}")
        if self_cond is not None and tuple(self_cond.shape) != tuple(y_t.shape):
            raise ValueError(f"self_cond must have the target's shape {tuple(y_t.shape)}, got {tuple(self_cond.shape)}")
        if level.numel() != B or angle.numel() != B or y_t.shape[0] != B or tuple(y_t.shape[2:]) != (H, W) or \
                (noise is not None and tuple(noise.shape) != tuple(y_t.shape)):
            raise ValueError(f"stack_views needs y_t (and noise) of shape {(B, 3, H, W)} and one level and angle per sample")
        if off.dtype != torch.int32 or off.numel() != B + 1 or rows > 65535:
            raise ValueError(f"off must be the int32 offsets table of {B} samples (ops.view_offsets), at most 65535 rows")
    elif drop is None and not null_rows:
        _call("vf_stack_views", _ptr(y_cond), _ptr(y_t), _ptr(noise), _ptr(level), _ptr(angle),
              ctypes.c_void_p(off.data_ptr()), _ptr(x), _ptr(ls), _ptr(as_), B, Nmax, Cc, H * W, S, int(copy_cond),
              _stream())
        return x, ls, as_
    if drop is not None:
        drop = _drop_mask(drop, B, y_cond.device)
    # the guided kernel, with or without the third part: vf_stack_views_sc takes self_cond in front of x
    _call("vf_stack_views_sc" if sc_on else "vf_stack_views_cfg", _ptr(y_cond), _ptr(y_t), _ptr(noise), _ptr(level),
          _ptr(angle), ctypes.c_void_p(off.data_ptr()), None if drop is None else ctypes.c_void_p(drop.data_ptr()),
          *((_ptr(self_cond),) if sc_on else ()), _ptr(x), _ptr(ls), _ptr(as_), B, Nmax, Cc, H * W, S, int(copy_cond),
          int(bool(null_rows)), _stream())
    return x, ls, as_


# ---- classifier-free guidance (csrc/diffusion.hip holds the definition) ----
def _drop_mask(drop, B, device):
    """A conditioning-dropout mask as the contiguous device uint8 (B,) the kernels read (bool is reinterpreted)."""
    if not torch.is_tensor(drop) or drop.dtype not in (torch.bool, torch.uint8) or drop.numel() != B:
        raise ValueError(f"a conditioning-dropout mask is a bool / uint8 tensor of {B} elements")
    if drop.device != device:
        raise _lib.VFHipError("the conditioning-dropout mask must live on the batch's device")
    drop = _c(drop.reshape(-1))
    return drop.view(torch.uint8) if drop.dtype == torch.bool else drop


def cond_drop_threshold(p):
    """thr = ceil(p * 2^24) of the seeded drop draw, p in [0, 1] (p * 2^24 is exact in double precision)."""
    p = float(p)
    if not 0.0 <= p <= 1.0:                      # (also refuses NaN)
        raise ValueError(f"the conditioning-dropout probability must be in [0, 1], got {p}")
    return int(math.ceil(p * 2.0 ** 24))


def draw_cond_drop(seed, ids, p):
    """The seeded conditioning-dropout mask of samples `ids`: device uint8 (B,), 1 = dropped.  A function of
    (seed, id) alone: word 2 of the call that gives the sample's t and u, against ceil(p * 2^24).  One launch."""
    thr = cond_drop_threshold(p)
    B = ids.numel()
    _check_ids(ids, B)
    drop = torch.empty(B, device=ids.device, dtype=torch.uint8)
    _call("vf_draw_cond_drop", _seed(seed), ctypes.c_void_p(ids.data_ptr()), thr, ctypes.c_void_p(drop.data_ptr()), B,
          _stream())
    return drop


def guidance_scales(device, B, guidance):
    """A guidance scale -- a number, or one per sample as a (B,) tensor / sequence -- as the contiguous fp32 (B,) tensor
    on `device` that the guided tails read.  Finite and >= 0, else ValueError (checked on the host: a device tensor is
    read back once, so hand the result, not the raw tensor, to anything that is called per step)."""
    if torch.is_tensor(guidance) or isinstance(guidance, (list, tuple)):
        g = torch.as_tensor(guidance).detach().reshape(-1).to(torch.float32)
        if g.numel() != B:
            raise ValueError(f"guidance needs one scale per sample: {g.numel()} scales for a batch of {B}")
        host = g.cpu()
        if not bool(torch.isfinite(host).all()) or bool((host < 0).any()):
            raise ValueError("guidance scales must be finite and >= 0")
        return _c(g.to(device))
    g = float(guidance)
    if not math.isfinite(g) or g < 0:
        raise ValueError(f"a guidance scale must be finite and >= 0, got {g}")
    return torch.full((B,), g, dtype=torch.float32, device=device)


def _check_guidance(guidance, unet_out, B, S):
    """The kernel reads row off[B] + b of unet_out and cannot see its row count: S = off[B] comes from the host
    (view_offsets), and unet_out must have exactly S + B rows."""
    _check(guidance)
    if guidance.numel() != B:
        raise ValueError(f"guidance needs one scale per sample (ops.guidance_scales): {guidance.numel()} for {B}")
    if S is None:
        raise ValueError("a guided tail needs S= (view_offsets): the null rows are rows S .. S + B - 1 of unet_out")
    if unet_out.shape[0] != int(S) + B:
        raise ValueError(f"a guided tail reads S + B rows (the null rows last): unet_out has {unet_out.shape[0]} rows "
                         f"for S = {int(S)} views of {B} samples")


# ---- dynamic thresholding / guidance rescaling (csrc/diffusion.hip holds the definition) ----
def quantile_position(n, q):
    """The two order statistics behind the q-quantile of n values, torch.quantile's linear interpolation:
    pos = q (n - 1) in float64, -> (k, frac) with k = floor(pos) and frac = float32(pos - k) in [0, 1); the quantile is
    x[k] + frac (x[k+1] - x[k]).  frac == 0 wherever x[k+1] would not exist (q = 1, n = 1); a frac that rounds to 1 in
    float32 is handed back as (k + 1, 0)."""
    n, q = int(n), float(q)
    if n < 1:
        raise ValueError(f"a quantile needs at least one value, got n = {n}")
    if not 0.0 <= q <= 1.0:                        # (also refuses NaN)
        raise ValueError(f"a quantile level must be in [0, 1], got {q}")
    pos = q * (n - 1)
    k = int(math.floor(pos))
    frac = struct.unpack("f", struct.pack("f", pos - k))[0]
    if frac >= 1.0:
        k, frac = k + 1, 0.0
    if k >= n - 1:
        k, frac = n - 1, 0.0
    return k, frac


def abs_quantile(x, q):
    """The q-quantile (q in [0, 1]) of |x| along the last dimension of a (B, n) tensor -> (B,), as
    torch.quantile(x.abs(), q, dim=1) defines it: exact radix selection of the two order statistics on the device, one
    workgroup per row, no sort, no host sync; the same bits on every call.  (The selection of the reverse step's dynamic
    threshold on a plain buffer; on its own e.g. a percentile stretch.)"""
    if x.dim() != 2:
        raise ValueError(f"abs_quantile takes a (B, n) tensor, got {tuple(x.shape)}")
    B, n = x.shape
    k, frac = quantile_position(n, q)
    x = _c(x)
    _check(x)
    out = torch.empty(B, device=x.device, dtype=torch.float32)
    _call("vf_abs_quantile", _ptr(x), B, n, k, frac, _ptr(out), _stream())
    return out


def threshold_settings(threshold=None, threshold_max=None, guidance_rescale=None, guided=False, clip=True):
    """The checked settings of a reverse step's dynamic threshold and guidance rescale -> (q | None, cmax, phi):
    q in (0, 1] the quantile level (None: off, the static clamp), cmax >= 1 the cap on the threshold (inf: none),
    phi in (0, 1] the rescale strength (0.0: off; guidance_rescale=0 is "off").  ValueError for anything else, for a
    rescale without guidance, a cap without a threshold, and a threshold with clip_denoised=False.  Host only."""
    q, cmax, phi = None, math.inf, 0.0
    if threshold is not None:
        q = float(threshold)
        if not 0.0 < q <= 1.0:
            raise ValueError(f"threshold (the quantile of |y0_hat|) must be in (0, 1], got {q}")
        if not clip:
            raise ValueError("threshold= replaces the clamp of y0_hat: it cannot be combined with clip_denoised=False")
    if threshold_max is not None:
        cmax = float(threshold_max)
        if not cmax >= 1.0:
            raise ValueError(f"threshold_max must be >= 1, got {cmax}")
        if q is None:
            raise ValueError("threshold_max= caps the dynamic threshold: it needs threshold=")
    if guidance_rescale is not None:
        phi = float(guidance_rescale)
        if not 0.0 <= phi <= 1.0:
            raise ValueError(f"guidance_rescale must be in [0, 1], got {phi}")
        if phi > 0.0 and not guided:
            raise ValueError("guidance_rescale= rescales the guided noise: it needs guidance=")
    return q, cmax, phi


def threshold_scratch(y):
    """What the thresholded / rescaled step keeps between its three launches, for a batch like y (B,3,H,W): the composed
    eps, the partial sums and stat = {r_b, s_b}.  generate() makes it once per call."""
    B = y.shape[0]
    return dict(eps=torch.empty_like(y), part=torch.empty(B * 64 * 4, device=y.device, dtype=torch.float64),
                stat=torch.empty(B, 2, device=y.device, dtype=torch.float32))


def _eps_front(unet_out, off, y, idx, ta, tb, B, max_views, weighting, wts, guidance, q, cmax, phi, scratch, fused):
    """The two launches in front of an *_eps tail: the composed (+ guided) eps with the weights (into wts | None) and
    the partial sums, then the per-sample statistics -> scratch.  fused: how that tail rounds y0_hat (the ancestral
    one fuses, the few-step one does not; csrc/diffusion.hip, y0_hat_as)."""
    _, Cout, H, W = unet_out.shape
    if scratch is None:
        scratch = threshold_scratch(y)
    eps, part, stat = scratch["eps"], scratch["part"], scratch["stat"]
    _check(eps, stat)
    if eps.shape != y.shape or stat.numel() != 2 * B or part.dtype != torch.float64 or part.numel() < B * 64 * 4 \
            or not part.is_cuda or not part.is_contiguous():
        raise ValueError("scratch= does not fit this batch (ops.threshold_scratch(y))")
    _call("vf_compose_eps", _ptr(unet_out), ctypes.c_void_p(off.data_ptr()), _ptr(guidance), _ptr(eps), _ptr(wts),
          ctypes.c_void_p(part.data_ptr()), B, Cout, H * W, max_views, int(weighting), int(fused), _stream())
    k, frac = (-1, 0.0) if q is None else quantile_position(3 * H * W, q)
    _call("vf_sample_stat", _ptr(eps), ctypes.c_void_p(part.data_ptr()), _ptr(y), ctypes.c_void_p(idx.data_ptr()),
          _ptr(ta), _ptr(tb), _ptr(stat), B, H * W, phi, k, frac, cmax, int(fused), _stream())
    return scratch


def _tail_noise(z, seed, ids, device, B):
    """The noise source of a tail -> (entry-point suffix, arguments): "" and z (None: no noise), or "_rng" and
    seed + ids for a draw inside the kernel."""
    if seed is None:
        return "", (_ptr(z),)
    ids = sample_ids(device, B, ids)
    _check_ids(ids, B)
    return "_rng", (_seed(seed), ctypes.c_void_p(ids.data_ptr()))


class _ComposeLossFn(torch.autograd.Function):
    """MSE(target, compose(unet_out)) fused: softmax over each sample's views (or mean)."""

    @staticmethod
    def forward(ctx, out, target, off, B, weighting):
        _check(out, target)
        S, Cout, H, W = out.shape
        nh = torch.empty(B, 3, H, W, device=out.device, dtype=torch.float32)
        part = torch.empty(B * 64 + 1, device=out.device, dtype=torch.float32)
        loss = part[B * 64:]
        _call("vf_compose_fwd", _ptr(out), ctypes.c_void_p(off.data_ptr()), _ptr(target), _ptr(nh), None,
                  _ptr(part), _ptr(loss), B, Cout, H * W, 0, int(weighting), _stream())
        ctx.save_for_backward(out, target, nh, off)
        ctx.B, ctx.weighting = B, int(weighting)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        out, target, nh, off = ctx.saved_tensors
        S, Cout, H, W = out.shape
        gloss = _c(gloss.reshape(1).float())
        # (the kernel writes channels 0..5; a wider output -- a learned-variance network trained without the vlb term --
        # gets zeros behind them)
        dout = torch.empty_like(out) if Cout <= 6 else torch.zeros_like(out)
        _call("vf_compose_mse_bwd", _ptr(out), ctypes.c_void_p(off.data_ptr()), _ptr(target), _ptr(nh),
                  _ptr(gloss), _ptr(dout), ctx.B, Cout, H * W, ctx.weighting, _stream())
        return dout, None, None, None, None


def compose_mse_loss(unet_out, target_noise, off, B, weighting):
    return _ComposeLossFn.apply(unet_out, _c(target_noise), off, B, weighting)


# ---- loss options (csrc/loss_weight.h): penalty x noise-level weight, per-sample loss, loss-by-level histogram ----
PENALTIES = {"mse": 0, "l1": 1, "huber": 2}
WEIGHT_KINDS = {None: 0, "none": 0, "min_snr": 1, "p2": 2, "trunc_snr": 3}


class _ComposeLossOptFn(torch.autograd.Function):
    """_ComposeLossFn with a penalty, a prediction, a per-sample weight of the noise level (times a per-sample scale) and
    the per-sample loss as a second (non-differentiable) output: the same two launches forward and one backward.
    pred 0 (eps): `target` is the ready-made target; pred 1 (v) | 2 (x0): it is the noise, and the kernels form the target
    from it, y_0 and level themselves -- no target buffer.
    vlb = (t, c1, hi, lo, lam) | None: the hybrid objective of a learned variance on a nine-channel output
    (csrc/diffusion.hip holds the definition), for every pred: loss = L_simple + lam mean_b vlb_b, the per-sample vlb
    (bits per dimension) a fourth non-differentiable output, and the backward writes all nine channels."""

    @staticmethod
    def forward(ctx, out, target, off, B, weighting, level, penalty, delta, kind, a, b, bin_sum, bin_cnt, scale=None,
                pred=0, y_0=None, vlb=None):
        t, c1, hi, lo, lam = vlb if vlb is not None else (None,) * 5
        _check(out, target, y_0, level, bin_sum, scale, c1, hi, lo)
        S, Cout, H, W = out.shape
        if level.numel() != B:
            raise ValueError(f"compose_loss needs one level per sample: {level.numel()} levels for a batch of {B}")
        if pred and (tuple(y_0.shape) != (B, 3, H, W) or tuple(target.shape) != (B, 3, H, W)):
            raise ValueError(f"compose_loss needs noise and y_0 of shape {(B, 3, H, W)}, got {tuple(target.shape)} and "
                             f"{tuple(y_0.shape)}")
        K = 0
        if bin_sum is not None:
            K = bin_sum.numel()
            if not bin_cnt.is_cuda or bin_cnt.dtype != torch.int32 or not bin_cnt.is_contiguous() or bin_cnt.numel() != K:
                raise _lib.VFHipError("hist must be (float32 [K], int32 [K]) contiguous device tensors")
        if scale is not None and scale.numel() != B:
            raise ValueError(f"compose_loss needs one scale per sample: {scale.numel()} for a batch of {B}")
        # nh: the composed prediction [| the composed o_b];  buf: partials [| vlb partials] | sample_loss | w (scale) |
        # [w] | [sample_vlb] | loss  (csrc/level_sampler.h; a scale and a vlb term never come together).  In floats:
        #   plain        nh (1,B,3,H,W)  buf 66 B + 1:   [0, 64B) | 64B | 65B | loss at 66B
        #   with scale   nh (1,B,3,H,W)  buf 67 B + 1:   [0, 64B) | 64B | 65B (w scale) | 66B (w) | loss at 67B
        #   with vlb     nh (2,B,3,H,W)  buf 131 B + 1:  [0, 64B) | [64B, 128B) | 128B | 129B | 130B (vlb) | loss at 131B
        # (nh always has the leading axis, so that the backward hands over one pointer per part)
        nv = 0 if vlb is None else 1
        nh = torch.empty(1 + nv, B, 3, H, W, device=out.device, dtype=torch.float32)
        s0 = B * 64 * (1 + nv)
        nw = 1 if scale is None else 2
        buf = torch.empty(s0 + B * (1 + nw + nv) + 1, device=out.device, dtype=torch.float32)
        sample_loss, sample_w, loss = buf[s0:s0 + B], buf[s0 + B:s0 + 2 * B], buf[s0 + B * (1 + nw + nv):]
        weight = sample_w if scale is None else buf[s0 + 2 * B:s0 + 3 * B]
        extra = ()
        # one entry point per path (the kernel log names them): each takes what its path has, in this order
        if vlb is not None:
            vlb_part, sample_vlb = buf[B * 64:s0], buf[s0 + 2 * B:s0 + 3 * B]
            tables = (ctypes.c_void_p(t.data_ptr()), _ptr(c1), _ptr(hi), _ptr(lo))
            entry, front, back = "vf_compose_loss_lv_fwd", (_ptr(target), _ptr(y_0), _ptr(level)) + tables, (pred, c1.numel(), lam)
            outs = (_ptr(nh[0]), _ptr(nh[1]), _ptr(buf), _ptr(vlb_part), _ptr(sample_loss), _ptr(sample_w), _ptr(sample_vlb))
            extra = (sample_vlb,)
        else:
            outs = (_ptr(nh), _ptr(buf), _ptr(sample_loss), _ptr(sample_w))
            if pred:
                entry, front, back = "vf_compose_loss_pred_fwd", (_ptr(target), _ptr(y_0), _ptr(level), _ptr(scale)), (pred,)
            elif scale is not None:
                entry, front, back = "vf_compose_loss_fwd_scaled", (_ptr(target), _ptr(level), _ptr(scale)), ()
            else:
                entry, front, back = "vf_compose_loss_fwd", (_ptr(target), _ptr(level)), ()
        _call(entry, _ptr(out), ctypes.c_void_p(off.data_ptr()), *front, *outs, _ptr(loss), _ptr(bin_sum),
              None if bin_cnt is None else ctypes.c_void_p(bin_cnt.data_ptr()),
              B, Cout, H * W, int(weighting), penalty, delta, kind, a, b, K, *back, _stream())
        ctx.save_for_backward(out, target, y_0, level, nh, off, sample_w, t, c1, hi, lo)
        ctx.B, ctx.weighting, ctx.penalty, ctx.delta, ctx.pred, ctx.lam = B, int(weighting), penalty, delta, pred, lam
        ctx.mark_non_differentiable(sample_loss, weight, *extra)
        return (loss.reshape(()), sample_loss, weight) + extra

    @staticmethod
    def backward(ctx, gloss, *_):
        out, target, y_0, level, nh, off, sample_w, t, c1, hi, lo = ctx.saved_tensors
        S, Cout, H, W = out.shape
        gloss = _c(gloss.reshape(1).float())
        # (without the vlb term the kernel writes channels 0..5, as in _ComposeLossFn.backward; with it all nine)
        dout = torch.empty_like(out) if Cout <= 6 or t is not None else torch.zeros_like(out)
        if t is not None:
            tables = (ctypes.c_void_p(t.data_ptr()), _ptr(c1), _ptr(hi), _ptr(lo))
            entry, front, back = "vf_compose_loss_lv_bwd", (_ptr(target), _ptr(y_0), _ptr(level)) + tables, (ctx.pred, c1.numel(), ctx.lam)
        elif ctx.pred:
            entry, front, back = "vf_compose_loss_pred_bwd", (_ptr(target), _ptr(y_0), _ptr(level)), (ctx.pred,)
        else:
            entry, front, back = "vf_compose_loss_bwd", (_ptr(target),), ()
        _call(entry, _ptr(out), ctypes.c_void_p(off.data_ptr()), *front, *(_ptr(h) for h in nh), _ptr(gloss),
              _ptr(sample_w), _ptr(dout), ctx.B, Cout, H * W, ctx.weighting, ctx.penalty, ctx.delta, *back, _stream())
        return (dout,) + (None,) * 16


def _check_nine(what, unet_out):
    if unet_out.dim() != 4 or unet_out.shape[1] != 9:
        raise ValueError(f"{what} needs a network output of 9 channels (prediction 0..2, logits 3..5, variance 6..8), "
                         f"got {unet_out.shape[1] if unet_out.dim() == 4 else tuple(unet_out.shape)} instead of 9")


def _compose_loss_lv(unet_out, target, off, B, weighting, level, penalty, delta, weight_kind, a, b, hist, prediction, y_0,
                     vlb):
    """The vlb= path of compose_loss: the checks, then _ComposeLossOptFn with the vlb tuple."""
    if not isinstance(vlb, (tuple, list)) or len(vlb) != 5:
        raise ValueError("vlb= takes (t, c1, hi, lo, weight)")
    t, c1, hi, lo, lam = vlb
    _check_nine("compose_loss(vlb=)", unet_out)
    lam = float(lam)
    if not math.isfinite(lam) or lam < 0:
        raise ValueError(f"the vlb weight must be finite and >= 0, got {lam}")
    _, _, H, W = unet_out.shape
    if level.numel() != B:
        raise ValueError(f"compose_loss needs one level per sample: {level.numel()} levels for a batch of {B}")
    if tuple(target.shape) != (B, 3, H, W) or (y_0 is not None and tuple(y_0.shape) != (B, 3, H, W)):
        raise ValueError(f"compose_loss needs a target / noise and y_0 of shape {(B, 3, H, W)}")
    if not (c1.numel() == hi.numel() == lo.numel()) or c1.numel() < 1:
        raise ValueError(f"vlb= needs c1, hi and lo of one length T, got {c1.numel()}, {hi.numel()} and {lo.numel()}")
    _check_i64("vlb's t", t, B)
    bin_sum, bin_cnt = hist if hist is not None else (None, None)
    return _ComposeLossOptFn.apply(unet_out, _c(target), off, B, weighting, _c(level.reshape(-1)), PENALTIES[penalty],
                                   float(delta), WEIGHT_KINDS[weight_kind], float(a), float(b), bin_sum, bin_cnt, None,
                                   PREDICTIONS[prediction], None if y_0 is None else _c(y_0),
                                   (t, _c(c1), _c(hi), _c(lo), lam))


def vlb_terms_host(o, hi, lo, c1, level, r, prediction="eps"):
    """The host mirror of csrc/vlb.h: float tensors / sequences of one length -> (lp, kl, dkl) float32 CPU tensors: the
    log-variance, KL in bits and dKL/dlp per element, m^2 = c1^2 kappa^2(level) r^2.  No GPU."""
    check_prediction(prediction)
    arrs = [torch.as_tensor(v, dtype=torch.float32).detach().cpu().reshape(-1).contiguous() for v in (o, hi, lo, c1, level, r)]
    n = arrs[0].numel()
    if any(v.numel() != n for v in arrs):
        raise ValueError("vlb_terms_host needs six inputs of one length")
    outs = [torch.empty(n, dtype=torch.float32) for _ in range(3)]
    rc = _lib.load().vf_vlb_terms_host(*(ctypes.c_void_p(v.data_ptr()) for v in arrs), PREDICTIONS[prediction],
                                       *(ctypes.c_void_p(v.data_ptr()) for v in outs), n)
    if rc != 0:
        raise _lib.VFHipError(f"vf_vlb_terms_host failed with {rc}")
    return tuple(outs)


# ---- prediction (csrc/diffusion.hip holds the definition): what channels 0..2 of the network mean ----
PREDICTIONS = {"eps": 0, "v": 1, "x0": 2}


def loss_weights_pred_host(level, prediction="eps", weight_kind=None, a=0.0, b=0.0):
    """The host mirror of the native loss weight (csrc/loss_weight.h): levels (any float tensor / sequence) -> float32
    CPU tensor of the same length.  No GPU."""
    check_prediction(prediction)
    if weight_kind not in WEIGHT_KINDS:
        raise ValueError(f"unknown loss weighting {weight_kind!r}: one of None, 'min_snr', 'p2', 'trunc_snr'")
    lv = torch.as_tensor(level, dtype=torch.float32).detach().cpu().reshape(-1).contiguous()
    out = torch.empty_like(lv)
    if weight_kind == "trunc_snr":             # a mirror of its own: the two older ones keep refusing codes above p2
        rc = _lib.load().vf_loss_weights_trunc_snr_host(ctypes.c_void_p(lv.data_ptr()), lv.numel(),
                                                        PREDICTIONS[prediction], ctypes.c_void_p(out.data_ptr()))
        if rc != 0:
            raise _lib.VFHipError(f"vf_loss_weights_trunc_snr_host failed with {rc}")
        return out
    rc = _lib.load().vf_loss_weights_pred_host(ctypes.c_void_p(lv.data_ptr()), lv.numel(), PREDICTIONS[prediction],
                                               WEIGHT_KINDS[weight_kind], float(a), float(b),
                                               ctypes.c_void_p(out.data_ptr()))
    if rc != 0:
        raise _lib.VFHipError(f"vf_loss_weights_pred_host failed with {rc}")
    return out


def compose_loss(unet_out, target, off, B, weighting, level, penalty="mse", delta=1.0, weight_kind=None, a=0.0, b=0.0,
                 hist=None, sample_scale=None, want_weight=False, prediction="eps", y_0=None, vlb=None):
    """compose_mse_loss with options: -> (loss, sample_loss).  d = compose(unet_out) - target;
    penalty "mse" d^2 | "l1" |d| | "huber" (F.huber_loss with `delta`);  sample_loss[b] = mean_i rho(d_bi) (B,), detached;
    weight_kind None | "min_snr" (w = min(1, a (1 - g) / g)) | "p2" (w = (a + g / (1 - g))^-b) | "trunc_snr"
    (w = max(1, (1 - g) / g)) of g = level[b], the sample's gamma (device float32 (B,));  loss = sum_b w_b sample_loss[b] / B, differentiable in unet_out.
    hist = (bin_sum float32 [K], bin_cnt int32 [K]) device accumulators: bin min(K - 1, int(g K)) receives the
    UNWEIGHTED sample_loss[b] and a count; they persist across calls (the caller zeroes them).
    sample_scale (device float32 (B,), default None: the launches above, untouched): a per-sample factor on w_b -- the
    importance weight of a non-uniform timestep draw (draw_level); loss = sum_b w_b scale_b sample_loss[b] / B, sample_loss
    and the histogram stay unweighted.
    want_weight=True: -> (loss, sample_loss, w) with w (B,) the noise-level weight ALONE (what level_stats reads).
    prediction "eps" (the default: everything above, launch for launch) | "v" | "x0" (csrc/diffusion.hip holds the
    definition): `target` is then the NOISE and y_0 (B, 3, H, W) is required; d = compose(unet_out) - the prediction's
    own target (v: sqrt(g) noise - sqrt(1 - g) y_0; x0: y_0), formed inside the loss kernels from noise, y_0 and level --
    no target buffer, the same launch count -- and w the prediction's native weight (csrc/loss_weight.h).
    vlb=(t, c1, hi, lo, weight) (default None: everything above, launch for launch): the hybrid objective of a learned
    variance (csrc/diffusion.hip holds the definition) on a NINE-channel unet_out -- loss = the loss above + weight
    mean_b vlb_b, vlb_b the mean over the sample's elements of KL(posterior || model) in bits, with the model's
    log-variance between lo[t] and hi[t] by the composed channels 6..8 and the residual d a constant inside it.  t: device
    int64 (B,); c1 (posterior_mean_coef1), hi, lo: device fp32 (T,) (schedule.variance_tables).  -> (loss, sample_loss,
    [w,] sample_vlb); the same launch count; the backward writes all nine channels.  No sample_scale."""
    if penalty not in PENALTIES:
        raise ValueError(f"unknown penalty {penalty!r}: one of {sorted(PENALTIES)}")
    if weight_kind not in WEIGHT_KINDS:
        raise ValueError(f"unknown loss weighting {weight_kind!r}: one of None, 'min_snr', 'p2', 'trunc_snr'")
    check_prediction(prediction)
    if prediction != "eps" and y_0 is None:
        raise ValueError(f"prediction {prediction!r} forms its target from the noise and y_0: y_0= is required")
    if prediction == "eps" and y_0 is not None:
        raise ValueError("y_0= belongs to prediction 'v' / 'x0' (with 'eps' the target is handed over ready-made)")
    if vlb is not None:
        if sample_scale is not None:
            raise ValueError("vlb= takes no sample_scale= (a level sampler with a learned variance is not built)")
        loss, sample_loss, weight, sample_vlb = _compose_loss_lv(unet_out, target, off, B, weighting, level, penalty, delta,
                                                                 weight_kind, a, b, hist, prediction, y_0, vlb)
        return (loss, sample_loss, weight, sample_vlb) if want_weight else (loss, sample_loss, sample_vlb)
    bin_sum, bin_cnt = hist if hist is not None else (None, None)
    if sample_scale is not None:
        sample_scale = _c(sample_scale.reshape(-1))
    loss, sample_loss, weight = _ComposeLossOptFn.apply(
        unet_out, _c(target), off, B, weighting, _c(level.reshape(-1)), PENALTIES[penalty], float(delta),
        WEIGHT_KINDS[weight_kind], float(a), float(b), bin_sum, bin_cnt, sample_scale, PREDICTIONS[prediction],
        None if y_0 is None else _c(y_0))
    return (loss, sample_loss, weight) if want_weight else (loss, sample_loss)


# ---- loss-aware noise-level sampling (csrc/level_sampler.h holds the specification) ----
LEVEL_MAX_BINS = 1024
LEVEL_KINDS = ("loss_aware", "fixed")


def level_table_host(q, T, K, uniform_mix):
    """The host mirror of the table: masses q (K,) -> (c int64 (K+1,), lo int32 (K+1,), iw float32 (K,)) CPU tensors."""
    q = torch.as_tensor(q, dtype=torch.float64).reshape(-1).contiguous()
    if q.numel() != K:
        raise ValueError(f"the proposal needs one mass per bin: {q.numel()} masses for {K} bins")
    c = torch.empty(K + 1, dtype=torch.int64)
    lo = torch.empty(K + 1, dtype=torch.int32)
    iw = torch.empty(K, dtype=torch.float32)
    rc = _lib.load().vf_level_table_host(ctypes.c_void_p(q.data_ptr()), int(T), int(K), float(uniform_mix),
                                         ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(lo.data_ptr()),
                                         ctypes.c_void_p(iw.data_ptr()))
    if rc != 0:
        raise ValueError("the proposal masses must be non-negative with a finite positive sum (and T, K, uniform_mix valid)")
    return c, lo, iw


def level_draw_host(x, T, K, c, iw):
    """The host mirror of the draw: words x (any integer tensor, values in [0, 2^32)) + table -> (t int64, iw float32)."""
    x = torch.as_tensor(x).reshape(-1).to(torch.int64)
    x32 = torch.from_numpy((x.numpy() & 0xFFFFFFFF).astype("uint32").view("int32"))      # the 32-bit patterns
    c, iw = c.to(torch.int64).contiguous(), iw.to(torch.float32).contiguous()
    t = torch.empty(x.numel(), dtype=torch.int64)
    w = torch.empty(x.numel(), dtype=torch.float32)
    rc = _lib.load().vf_level_draw_host(ctypes.c_void_p(x32.data_ptr()), x.numel(), int(T), int(K),
                                        ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(iw.data_ptr()),
                                        ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(w.data_ptr()))
    if rc != 0:
        raise ValueError("not a proposal table: c must rise strictly from 0 to 2^32 over K + 1 entries")
    return t, w


def check_level_sampler(kind, T, bins, probs, ema, warmup, uniform_mix):
    """The checked settings of a level sampler -> (K, probs | None as a float64 CPU tensor, ema, warmup, uniform_mix);
    ValueError for anything else.  Host only, no GPU."""
    if kind not in LEVEL_KINDS:
        raise ValueError(f"unknown level sampler {kind!r}: one of None, 'loss_aware', 'fixed'")
    if isinstance(bins, bool) or not isinstance(bins, int) or bins < 1:
        raise ValueError(f"bins must be a positive integer, got {bins!r}")
    if bins > min(T - 1, LEVEL_MAX_BINS):
        raise ValueError(f"bins must be at most min(T - 1, {LEVEL_MAX_BINS}) = {min(T - 1, LEVEL_MAX_BINS)}, got {bins}")
    ema, uniform_mix = float(ema), float(uniform_mix)
    if not 0.0 <= ema < 1.0:
        raise ValueError(f"ema must be in [0, 1), got {ema}")
    if isinstance(warmup, bool) or not isinstance(warmup, int) or warmup < 0:
        raise ValueError(f"warmup must be a non-negative integer, got {warmup!r}")
    if not uniform_mix <= 1.0 or uniform_mix * 2.0 ** 32 < 2 * (T - 1):
        raise ValueError(f"uniform_mix must be in [2 (T - 1) / 2^32, 1] = [{2 * (T - 1) / 2.0 ** 32:.3g}, 1] so that every "
                         f"timestep keeps at least one word, got {uniform_mix}")
    if kind == "fixed":
        if probs is None:
            raise ValueError("a 'fixed' level sampler needs probs= (one mass per bin)")
        probs = torch.as_tensor(probs, dtype=torch.float64).detach().cpu().reshape(-1)
        if probs.numel() != bins:
            raise ValueError(f"probs needs one mass per bin: {probs.numel()} masses for {bins} bins")
        if not bool(torch.isfinite(probs).all()) or bool((probs < 0).any()):
            raise ValueError("probs must be finite and non-negative")
        if not float(probs.sum()) > 0:
            raise ValueError("probs must not be all zero")
    elif probs is not None:
        raise ValueError("probs= belongs to the 'fixed' level sampler")
    return bins, probs, ema, warmup, uniform_mix


class LevelSampler:
    """The device state of a noise-level sampler over T timesteps in K bins (csrc/level_sampler.h): the proposal table
    c int64 (K+1,) / iw float32 (K,), ready int32 (1,) and, for "loss_aware", the statistics m float32 (K,) /
    seen int32 (K,).  "fixed": the table of `probs`, normalised by the host mirror, ready from the start and never
    updated.  "loss_aware": starts not ready (the uniform draw, weight 1) with a uniform table; level_stats() feeds it.
    The tensors are updated in place for the sampler's whole life: captured launches address them."""

    def __init__(self, kind, T, device, bins, probs=None, ema=0.9, warmup=10, uniform_mix=0.01):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("a level sampler lives on the GPU (its draw and statistics are HIP kernels)")
        K, probs, ema, warmup, uniform_mix = check_level_sampler(kind, int(T), bins, probs, ema, warmup, uniform_mix)
        self.kind, self.T, self.K, self.ema, self.warmup, self.uniform_mix = kind, int(T), K, ema, warmup, uniform_mix
        c, lo, iw = level_table_host(torch.ones(K, dtype=torch.float64) if probs is None else probs, self.T, K, uniform_mix)
        self.n = (lo[1:] - lo[:-1]).to(device)
        self.c, self.iw = c.to(device), iw.to(device)
        self.ready = torch.full((1,), int(kind == "fixed"), dtype=torch.int32, device=device)
        self.m = torch.zeros(K, dtype=torch.float32, device=device)
        self.seen = torch.zeros(K, dtype=torch.int32, device=device)

    def proposal(self):
        """-> (p (K,) float64: the bin masses width_k / 2^32 of the table as it stands, or n_k / (T - 1) while not ready;
        seen (K,) int32; ready (1,) bool).  Device tensors, no sync."""
        p = (self.c[1:] - self.c[:-1]).to(torch.float64) / 2.0 ** 32
        ready = self.ready != 0
        return torch.where(ready, p, self.n.to(torch.float64) / (self.T - 1)), self.seen.clone(), ready

    def state_dict(self):
        return dict(kind=self.kind, T=self.T, bins=self.K, ema=self.ema, warmup=self.warmup, uniform_mix=self.uniform_mix,
                    c=self.c.cpu(), iw=self.iw.cpu(), ready=self.ready.cpu(), m=self.m.cpu(), seen=self.seen.cpu())

    def load_state_dict(self, sd):
        for k, mine in (("kind", self.kind), ("T", self.T), ("bins", self.K)):
            if sd[k] != mine:
                raise ValueError(f"the saved level sampler has {k} = {sd[k]!r}, this one {mine!r}")
        c = torch.as_tensor(sd["c"]).to(torch.int64).cpu()
        if c.numel() != self.K + 1 or int(c[0]) != 0 or int(c[-1]) != 1 << 32 or not bool((c[1:] > c[:-1]).all()):
            raise ValueError("the saved proposal table does not rise strictly from 0 to 2^32 over bins + 1 entries")
        self.ema, self.warmup, self.uniform_mix = float(sd["ema"]), int(sd["warmup"]), float(sd["uniform_mix"])
        self.c.copy_(c)
        for name in ("iw", "ready", "m", "seen"):
            dst = getattr(self, name)
            dst.copy_(torch.as_tensor(sd[name]).to(dst.dtype).reshape(dst.shape))


def draw_level(sampler, gammas, seed=None, ids=None, words=None, want_u=False):
    """draw_train through a LevelSampler's table: -> (t (B,) int64, level (B,) | None, u (B,) | None, iw (B,) float32).
    Either seed + ids (word 0 of the sample's training-scalars call picks t; u and level as draw_train) or words, a device
    int64 (B,) of values in [0, 2^32) (the unseeded path: level and u are None, the caller draws u).  While the sampler
    is not ready: draw_train's t and iw = 1.  One launch, no host sync."""
    _check(gammas)
    if gammas.numel() != sampler.T:
        raise ValueError(f"the level sampler was built for T = {sampler.T}, the schedule has {gammas.numel()} levels")
    if (seed is None) == (words is None):
        raise ValueError("draw_level takes either seed= (with ids=) or words=")
    dev = gammas.device
    if words is None:
        B = ids.numel()
        _check_ids(ids, B)
        src = (_seed(seed), ctypes.c_void_p(ids.data_ptr()), None)
    else:
        B = words.numel()
        if not words.is_cuda or words.dtype != torch.int64 or not words.is_contiguous():
            raise _lib.VFHipError("words must be a contiguous device int64 tensor (values in [0, 2^32))")
        src = (0, None, ctypes.c_void_p(words.data_ptr()))
    t = torch.empty(B, device=dev, dtype=torch.int64)
    iw = torch.empty(B, device=dev, dtype=torch.float32)
    level = torch.empty(B, device=dev, dtype=torch.float32) if words is None else None
    u = torch.empty(B, device=dev, dtype=torch.float32) if (want_u and words is None) else None
    _call("vf_draw_level", *src, _ptr(gammas), sampler.T, sampler.K, ctypes.c_void_p(sampler.c.data_ptr()),
          _ptr(sampler.iw), ctypes.c_void_p(sampler.ready.data_ptr()), ctypes.c_void_p(t.data_ptr()), _ptr(u),
          _ptr(level), _ptr(iw), B, _stream())
    return t, level, u, iw


def level_stats(sampler, sample_loss, sample_w, t):
    """One step's statistics into a "loss_aware" sampler, then its table: r_b = (sample_w[b] sample_loss[b])^2 into
    bin(t[b]) (sample_w None: 1; it is the noise-level weight ALONE), EMA per bin, ready / c / iw rebuilt on the device.
    One one-workgroup launch, no host sync, no atomics."""
    if sampler.kind != "loss_aware":
        raise ValueError("only a 'loss_aware' level sampler keeps statistics")
    _check(sample_loss, sample_w)
    B = sample_loss.numel()
    if not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != B or \
            (sample_w is not None and sample_w.numel() != B):
        raise _lib.VFHipError(f"level_stats needs t (contiguous device int64) and sample_w with {B} elements each")
    _call("vf_level_stats", _ptr(sample_loss), _ptr(sample_w), ctypes.c_void_p(t.data_ptr()), B, sampler.T, sampler.K,
          sampler.ema, sampler.warmup, sampler.uniform_mix, _ptr(sampler.m),
          ctypes.c_void_p(sampler.seen.data_ptr()), ctypes.c_void_p(sampler.c.data_ptr()), _ptr(sampler.iw),
          ctypes.c_void_p(sampler.ready.data_ptr()), _stream())


def compose(unet_out, off, B, max_views, weighting, want_weights=True):
    """Inference compose: -> noise (B,3,H,W), weights (B,maxV,3,H,W) | None."""
    _check(unet_out)
    S, Cout, H, W = unet_out.shape
    nh = torch.empty(B, 3, H, W, device=unet_out.device, dtype=torch.float32)
    wts = None
    if weighting and want_weights:
        wts = torch.empty(B, max_views, 3, H, W, device=unet_out.device, dtype=torch.float32)
    _call("vf_compose_fwd", _ptr(unet_out), ctypes.c_void_p(off.data_ptr()), None, _ptr(nh), _ptr(wts), None,
              None, B, Cout, H * W, max_views, int(weighting), _stream())
    return nh, wts


def p_sample_tail(unet_out, off, y_t, z, t, sched, B, max_views, weighting, clip=True, want_weights=True,
                  want_mean=False, inplace=False, seed=None, ids=None, guidance=None, S=None, threshold=None,
                  threshold_max=None, guidance_rescale=None, scratch=None):
    """Fused compose -> y0_hat -> clamp -> posterior mean -> + z*sigma.
    Returns (y_next, mean | None, weights | None).  seed= (with z=None): z is drawn inside the kernel from
    (seed, ids[b], t[b], element) and is 0 where t[b] == 0; ids defaults to arange(B).
    guidance (device fp32 (B,), ops.guidance_scales) with S= (view_offsets' S = off[B], checked against unet_out's row
    count): unet_out has S + B rows, the null rows last, and the composed noise is g eps_c + (1 - g) eps_u
    (classifier-free guidance); the weights stay the conditional ones.
    threshold (q in (0, 1], optional threshold_max >= 1) / guidance_rescale (phi in (0, 1], needs guidance): dynamic
    thresholding of y0_hat in place of the static clamp / the guided noise rescaled to the conditional one's standard
    deviation (csrc/diffusion.hip holds the definition).  Either one runs three launches instead of one -- the composed
    eps (+ weights), the per-sample statistics, the tail on the eps buffer; scratch= (ops.threshold_scratch) lets a loop
    allocate their buffers once."""
    q, cmax, phi = threshold_settings(threshold, threshold_max, guidance_rescale, guidance is not None, clip)
    _check(unet_out, y_t, z)
    if guidance is not None:
        _check_guidance(guidance, unet_out, B, S)
    if seed is not None and z is not None:
        raise ValueError("p_sample_tail takes either z or seed=, not both")
    t = _c(t.to(torch.int64))
    y_next = y_t if inplace else torch.empty_like(y_t)     # elementwise: safe to overwrite y_t
    mean = torch.empty_like(y_t) if want_mean else None
    _, Cout, H, W = unet_out.shape
    tabs = [sched[n] for n in ("sqrt_recip_gammas", "sqrt_recipm1_gammas", "posterior_log_variance_clipped",
                               "posterior_mean_coef1", "posterior_mean_coef2")]
    wts = None
    if weighting and want_weights:
        wts = torch.empty(B, max_views, 3, H, W, device=y_t.device, dtype=torch.float32)
    # the entry point: vf_p_sample_tail + the source of eps ("" | "_cfg" | "_eps") + the source of z ("" | "_rng")
    if q is not None or phi > 0.0:
        scratch = _eps_front(unet_out, off, y_t, t, tabs[0], tabs[1], B, max_views, weighting, wts, guidance, q, cmax,
                             phi, scratch, True)
        eps, src = "_eps", (_ptr(scratch["eps"]), _ptr(scratch["stat"]))
        sizes = (B, H * W, int(clip), int(phi > 0.0), int(q is not None))
    else:
        eps, src = "" if guidance is None else "_cfg", (_ptr(unet_out), ctypes.c_void_p(off.data_ptr()))
        sizes = (_ptr(wts), B, Cout, H * W, max_views, int(weighting), int(clip),
                 *(() if guidance is None else (_ptr(guidance),)))
    rng, noise = _tail_noise(z, seed, ids, y_t.device, B)
    _call(f"vf_p_sample_tail{eps}{rng}", *src, _ptr(y_t), *noise, ctypes.c_void_p(t.data_ptr()),
          *(_ptr(tab) for tab in tabs), _ptr(y_next), _ptr(mean), *sizes, _stream())
    return y_next, mean, wts


def sampler_step(unet_out, off, y, z, kidx, tables, B, max_views, weighting, y0_prev=None, want_weights=True,
                 inplace=False, seed=None, ids=None, guidance=None, S=None, threshold=None, threshold_max=None,
                 guidance_rescale=None, scratch=None, variance=None, want_logvar=False):
    """One step of a few-step sampler (strided DDIM / DPM-Solver++ 2M), fused like p_sample_tail:
    compose -> y0 = clamp(a[k] y - b[k] eps) -> y_new = cy[k] y + c0[k] y0 + c1[k] y0_prev + sigma[k] z, k = kidx[b].
    tables: the fp32 device tables a, b, cy, c0, c1, sigma (K,) and tau (K,) int64 (ViewFusion._sampler_plan).
    y0_prev (like y, optional): the multistep history, updated in place; it is not read where c1[k] == 0.
    Returns (y_next, weights | None).  seed= (with z=None): z is drawn inside the kernel from
    (seed, ids[b], tau[k], element); where sigma[k] == 0 no z is loaded or drawn at all.
    guidance (device fp32 (B,)) with S=: the guided tail, as in p_sample_tail.
    threshold / threshold_max / guidance_rescale / scratch: as in p_sample_tail; y0_prev receives the thresholded y0.
    variance=(hi, lo) (default None: everything above, launch for launch): the learned-variance step (csrc/diffusion.hip
    holds the definition) on a NINE-channel unet_out and the "ddim", eta = 1 tables -- where sigma[k] != 0 the noise
    scale is expf(0.5 lp) per element, lp between lo[k] and hi[k] (device fp32 (K,), schedule.variance_tables) by the
    composed channels 6..8 of the conditional rows; no history term and no threshold / rescale flavour.
    want_logvar=True (with variance=): -> (y_next, weights | None, lp (B,3,H,W))."""
    q, cmax, phi = threshold_settings(threshold, threshold_max, guidance_rescale, guidance is not None)
    if variance is not None:
        return _sampler_step_lv(unet_out, off, y, z, kidx, tables, B, max_views, weighting, y0_prev, want_weights, inplace,
                                seed, ids, guidance, S, q is not None or phi > 0.0, variance, want_logvar)
    if want_logvar:
        raise ValueError("want_logvar= belongs to the learned-variance step: it needs variance=(hi, lo)")
    _check(unet_out, y, z, y0_prev, *(tables[n] for n in ("a", "b", "cy", "c0", "c1", "sigma")))
    if guidance is not None:
        _check_guidance(guidance, unet_out, B, S)
    if seed is not None and z is not None:
        raise ValueError("sampler_step takes either z or seed=, not both")
    kidx = _c(kidx.to(torch.int64))
    y_next = y if inplace else torch.empty_like(y)         # elementwise: safe to overwrite y
    _, Cout, H, W = unet_out.shape
    tabs = [tables[n] for n in ("a", "b", "cy", "c0", "c1", "sigma")]
    wts = None
    if weighting and want_weights:
        wts = torch.empty(B, max_views, 3, H, W, device=y.device, dtype=torch.float32)
    # the entry point: vf_sampler_step + the source of eps ("" | "_cfg" | "_eps") + the source of z ("" | "_rng")
    if q is not None or phi > 0.0:
        scratch = _eps_front(unet_out, off, y, kidx, tabs[0], tabs[1], B, max_views, weighting, wts, guidance, q, cmax,
                             phi, scratch, False)
        eps, src = "_eps", (_ptr(scratch["eps"]), _ptr(scratch["stat"]))
        sizes = (B, H * W, int(phi > 0.0), int(q is not None))
    else:
        eps, src = "" if guidance is None else "_cfg", (_ptr(unet_out), ctypes.c_void_p(off.data_ptr()))
        sizes = (_ptr(wts), B, Cout, H * W, max_views, int(weighting), *(() if guidance is None else (_ptr(guidance),)))
    rng, noise = _tail_noise(z, seed, ids, y.device, B)
    idx = (ctypes.c_void_p(kidx.data_ptr()),)
    if rng:                                                # the drawn z is keyed by the model timestep tau[k]
        tau = tables["tau"]
        if not tau.is_cuda or tau.dtype != torch.int64 or not tau.is_contiguous():
            raise _lib.VFHipError("tables['tau'] must be a contiguous device int64 tensor")
        idx += (ctypes.c_void_p(tau.data_ptr()),)
    _call(f"vf_sampler_step{eps}{rng}", *src, _ptr(y), *noise, *idx, *(_ptr(tab) for tab in tabs), _ptr(y0_prev),
          _ptr(y_next), *sizes, _stream())
    return y_next, wts


def _sampler_step_lv(unet_out, off, y, z, kidx, tables, B, max_views, weighting, y0_prev, want_weights, inplace, seed, ids,
                     guidance, S, dynamic, variance, want_logvar):
    """The variance= path of sampler_step: the checks, then one of the four vf_sampler_step_lv* entries."""
    if not isinstance(variance, (tuple, list)) or len(variance) != 2:
        raise ValueError("variance= takes (hi, lo)")
    if dynamic:
        raise ValueError("threshold= / guidance_rescale= with a learned variance are not built: the tails on the eps "
                         "buffer carry no variance")
    hi, lo = variance
    tabs = [tables[n] for n in ("a", "b", "cy", "c0", "sigma")]
    _check(unet_out, y, z, y0_prev, hi, lo, *tabs)
    _check_nine("sampler_step(variance=)", unet_out)
    K = tabs[0].numel()
    if any(tab.numel() != K for tab in tabs) or hi.numel() != K or lo.numel() != K:
        raise ValueError(f"variance= needs hi and lo of the chain's length {K}, got {hi.numel()} and {lo.numel()}")
    if "c1" in tables and bool(tables.get("multistep", False)):
        raise ValueError("the learned-variance step has no history term: it runs on the 'ddim' tables")
    if guidance is not None:
        _check_guidance(guidance, unet_out, B, S)
    if seed is not None and z is not None:
        raise ValueError("sampler_step takes either z or seed=, not both")
    _, Cout, H, W = unet_out.shape
    if tuple(y.shape) != (B, 3, H, W):
        raise ValueError(f"sampler_step needs y of shape {(B, 3, H, W)}, got {tuple(y.shape)}")
    kidx = _c(kidx.to(torch.int64))
    y_next = y if inplace else torch.empty_like(y)
    wts = None
    if weighting and want_weights:
        wts = torch.empty(B, max_views, 3, H, W, device=y.device, dtype=torch.float32)
    lp = torch.empty_like(y) if want_logvar else None
    rng, noise = _tail_noise(z, seed, ids, y.device, B)
    idx = (ctypes.c_void_p(kidx.data_ptr()),)
    if rng:
        tau = tables["tau"]
        if not tau.is_cuda or tau.dtype != torch.int64 or not tau.is_contiguous() or tau.numel() != K:
            raise _lib.VFHipError(f"tables['tau'] must be a contiguous device int64 tensor of {K} elements")
        idx += (ctypes.c_void_p(tau.data_ptr()),)
    cfg = "" if guidance is None else "_cfg"
    _call(f"vf_sampler_step_lv{cfg}{rng}", _ptr(unet_out), ctypes.c_void_p(off.data_ptr()), _ptr(y), *noise, *idx,
          *(_ptr(tab) for tab in tabs), _ptr(hi), _ptr(lo), _ptr(y0_prev), _ptr(y_next), _ptr(wts), _ptr(lp), B, Cout,
          H * W, max_views, int(weighting), *(() if guidance is None else (_ptr(guidance),)), _stream())
    return (y_next, wts, lp) if want_logvar else (y_next, wts)


# ---- progressive distillation (csrc/diffusion.hip holds the definition) ----
def _check_i64(name, t, n):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != n:
        raise _lib.VFHipError(f"{name} must be a contiguous device int64 tensor of {n} elements")


def distill_step_host(seed, ids, K):
    """The host mirror of the seeded draw of a distillation sample's student step: ids (any integer tensor / sequence)
    -> int64 CPU tensor, i = mulhi32(word 0 of the sample's training-scalars call, K) in [0, K).  No GPU."""
    K = int(K)
    ids = torch.as_tensor(ids).detach().cpu().reshape(-1).to(torch.int64).contiguous()
    out = torch.empty_like(ids)
    rc = _lib.load().vf_distill_step_host(_seed(seed), ctypes.c_void_p(ids.data_ptr()), K,
                                          ctypes.c_void_p(out.data_ptr()), ids.numel())
    if rc != 0:
        raise ValueError(f"the student's step count must be in [1, 2^27], got {K}")
    return out


def distill_begin(y_0, noise, tau_s, gammas, seed=None, ids=None, i=None):
    """The head of a distillation sample batch, one launch: -> (i, k1, k0 int64 (B,), level_s (B,), z_t like y_0).
    i = the student step of each sample: `i` (device int64 (B,), clamped to [0, K)) when given, else the seeded draw
    mulhi32(word 0, K) of samples `ids` (ops.sample_ids); k1 = 2 i + 1 and k0 = 2 i index the teacher's 2K-step tables;
    level_s = gammas[tau_s[i]], tau_s the student's K model timesteps (device int64 (K,));
    z_t = sqrt(level_s) y_0 + sqrt(1 - level_s) noise."""
    y_0, noise = _c(y_0), _c(noise)
    _check(y_0, noise, gammas)
    if y_0.dim() != 4 or y_0.shape[1] != 3 or noise.shape != y_0.shape:
        raise ValueError(f"distill_begin takes y_0 and noise of one (B, 3, H, W) shape, got {tuple(y_0.shape)} and "
                         f"{tuple(noise.shape)}")
    B = y_0.shape[0]
    n = y_0[0].numel()
    if n % 4:
        raise ValueError(f"H W must be a multiple of 4, got {tuple(y_0.shape)}")
    K = tau_s.numel()
    _check_i64("tau_s", tau_s, K)
    if K < 1 or K > gammas.numel():
        raise ValueError(f"tau_s holds the student's K model timesteps, 1 <= K <= T: got {K} for T = {gammas.numel()}")
    if (i is None) == (seed is None):
        raise ValueError("distill_begin takes either i= or seed= (with ids=)")
    if i is None:
        ids = sample_ids(y_0.device, B, ids)
        _check_ids(ids, B)
        src = (_seed(seed), ctypes.c_void_p(ids.data_ptr()), None)
    else:
        i = _c(i.reshape(-1))
        _check_i64("i", i, B)
        src = (0, None, ctypes.c_void_p(i.data_ptr()))
    idx = torch.empty(3, B, device=y_0.device, dtype=torch.int64)
    level_s = torch.empty(B, device=y_0.device, dtype=torch.float32)
    z_t = torch.empty_like(y_0)
    _call("vf_distill_begin", *src, ctypes.c_void_p(tau_s.data_ptr()), _ptr(gammas), K, _ptr(y_0), _ptr(noise),
          ctypes.c_void_p(idx[0].data_ptr()), ctypes.c_void_p(idx[1].data_ptr()), ctypes.c_void_p(idx[2].data_ptr()),
          _ptr(level_s), _ptr(z_t), B, n, _stream())
    return idx[0], idx[1], idx[2], level_s, z_t


def distill_target(unet_out, off, y, x1, z_t, level_s, i, k0, tables, w1, w2, B, weighting, guidance=None, S=None):
    """The second teacher step's tail and the student's target, one launch: -> (x_tilde, eps_tilde), both like y.
    unet_out: the teacher's output at y = z' (S rows, or S + B with guidance: the null rows last); x1: the history buffer
    the first teacher step (sampler_step(y0_prev=x1)) wrote; z_t, level_s, i, k0: distill_begin's; tables: the teacher's
    fp32 device tables a, b (2K,); w1, w2: fp32 device (K,) (schedule.distill_tables).
    x2 = clamp(a[k0] y - b[k0] out2, -1, 1), x_tilde = clamp(w1[i] x1 + w2[i] x2, -1, 1),
    eps_tilde = (z_t - sqrt(level_s) x_tilde) / sqrt(1 - level_s).  guidance (device fp32 (B,)) with S=: as sampler_step."""
    _check(unet_out, y, x1, z_t, level_s, tables["a"], tables["b"], w1, w2)
    if unet_out.dim() != 4 or y.dim() != 4 or y.shape[0] != B or y.shape[1] != 3 or x1.shape != y.shape or \
            z_t.shape != y.shape or unet_out.shape[-2:] != y.shape[-2:]:
        raise ValueError(f"distill_target takes y, x1 and z_t of one ({B}, 3, H, W) shape and unet_out (rows, C, H, W), got "
                         f"{tuple(y.shape)}, {tuple(x1.shape)}, {tuple(z_t.shape)} and {tuple(unet_out.shape)}")
    if guidance is not None:
        _check_guidance(guidance, unet_out, B, S)
    elif S is not None and unet_out.shape[0] != int(S):
        raise ValueError(f"unet_out has {unet_out.shape[0]} rows for S = {int(S)} views")
    _, Cout, H, W = unet_out.shape
    if (H * W) % 4 or Cout < (6 if weighting else 3):
        raise ValueError(f"distill_target needs H W % 4 == 0 and {6 if weighting else 3} output channels, got "
                         f"{tuple(unet_out.shape)}")
    K = w1.numel()
    if w2.numel() != K or tables["a"].numel() != 2 * K or tables["b"].numel() != 2 * K or level_s.numel() != B:
        raise ValueError("distill_target needs w1, w2 of K entries, teacher tables of 2K entries and one level per sample")
    _check_i64("i", i, B)
    _check_i64("k0", k0, B)
    if off.dtype != torch.int32 or off.numel() != B + 1:
        raise ValueError(f"off must be the int32 offsets table of {B} samples (ops.view_offsets)")
    x_t, e_t = torch.empty_like(y), torch.empty_like(y)
    _call("vf_distill_target", _ptr(unet_out), ctypes.c_void_p(off.data_ptr()), _ptr(y), _ptr(x1), _ptr(z_t),
          _ptr(level_s), ctypes.c_void_p(i.data_ptr()), ctypes.c_void_p(k0.data_ptr()), _ptr(tables["a"]),
          _ptr(tables["b"]), _ptr(w1), _ptr(w2), _ptr(x_t), _ptr(e_t), B, Cout, H * W, int(weighting), _ptr(guidance),
          _stream())
    return x_t, e_t


# ---- self-conditioning (csrc/diffusion.hip holds the definition) ----
def self_cond_threshold(p):
    """thr = ceil(p * 2^24) of the seeded self-conditioning coin, p in [0, 1] (p * 2^24 is exact in double precision)."""
    p = float(p)
    if not 0.0 <= p <= 1.0:                      # (also refuses NaN)
        raise ValueError(f"the self-conditioning probability must be in [0, 1], got {p}")
    return int(math.ceil(p * 2.0 ** 24))


def draw_self_cond(seed, ids, p):
    """The seeded self-conditioning coin of samples `ids`: device uint8 (B,), 1 = the estimate is fed back.  A function
    of (seed, id) alone: word 3 of the call that gives the sample's t, u and conditioning drop, against ceil(p * 2^24).
    One launch."""
    thr = self_cond_threshold(p)
    B = ids.numel()
    _check_ids(ids, B)
    keep = torch.empty(B, device=ids.device, dtype=torch.uint8)
    _call("vf_draw_self_cond", _seed(seed), ctypes.c_void_p(ids.data_ptr()), thr, ctypes.c_void_p(keep.data_ptr()), B,
          _stream())
    return keep


def self_cond_draw_host(seed, ids, p):
    """The host mirror of draw_self_cond: ids (any integer tensor / sequence) -> uint8 CPU tensor.  No GPU."""
    thr = self_cond_threshold(p)
    ids = torch.as_tensor(ids).detach().cpu().reshape(-1).to(torch.int64).contiguous()
    out = torch.empty(ids.numel(), dtype=torch.uint8)
    rc = _lib.load().vf_self_cond_draw_host(_seed(seed), ctypes.c_void_p(ids.data_ptr()), thr,
                                            ctypes.c_void_p(out.data_ptr()), ids.numel())
    if rc != 0:
        raise _lib.VFHipError(f"vf_self_cond_draw_host failed with {rc}")
    return out


def self_cond_coeffs_host(level, prediction="eps"):
    """The host mirror of the estimate's coefficients: levels -> (a, b) float32 CPU tensors of x^ = a y_t - b out.  No GPU."""
    check_prediction(prediction)
    lv = torch.as_tensor(level, dtype=torch.float32).detach().cpu().reshape(-1).contiguous()
    a, b = torch.empty_like(lv), torch.empty_like(lv)
    rc = _lib.load().vf_self_cond_coeffs_host(ctypes.c_void_p(lv.data_ptr()), PREDICTIONS[prediction],
                                              ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), lv.numel())
    if rc != 0:
        raise _lib.VFHipError(f"vf_self_cond_coeffs_host failed with {rc}")
    return a, b


def self_cond_estimate(unet_out, off, level, B, weighting, prediction="eps", x=None, y_t=None, keep=None):
    """The self-conditioning estimate of a first pass, one launch: -> x^ (B,3,H,W) = keep_b clamp(a(g) y_t - b(g) out_b, -1, 1),
    out_b the composition of unet_out (S rows) over the sample's views (weighting: softmax of channels 3..5, else the
    mean), g = level[b] (device fp32 (B,)).  y_t is read back from the stacked input x (S,Cc+6,H,W) the pass saw -- its
    channels Cc..Cc+2 in the sample's first row -- or from a plain y_t (B,3,H,W); "x0" reads neither.  keep (device
    bool / uint8 (B,), default None: every sample): a sample with keep = 0 gets exact zeros."""
    check_prediction(prediction)
    _check(unet_out, level, x, y_t)
    if unet_out.dim() != 4:
        raise ValueError(f"self_cond_estimate takes unet_out (S, C, H, W), got {tuple(unet_out.shape)}")
    S, Cout, H, W = unet_out.shape
    HW = H * W
    if HW % 4 or Cout < (6 if weighting else 3):
        raise ValueError(f"self_cond_estimate needs H W % 4 == 0 and {6 if weighting else 3} output channels, got "
                         f"{tuple(unet_out.shape)}")
    if off.dtype != torch.int32 or off.numel() != B + 1 or not off.is_cuda or level.numel() != B or B > 65535:
        raise ValueError(f"self_cond_estimate needs the int32 offsets table of {B} samples (ops.view_offsets) and one level "
                         "per sample")
    src, stride, choff, by_view = None, 0, 0, 0
    if prediction != "x0":
        if (x is None) == (y_t is None):
            raise ValueError("self_cond_estimate reads y_t from exactly one of x= (the stacked input) and y_t=")
        if x is not None:
            if x.dim() != 4 or x.shape[0] < S or x.shape[1] < 7 or tuple(x.shape[2:]) != (H, W):
                raise ValueError(f"x must be the self-conditioned stacked input (rows >= {S}, Cc + 6, {H}, {W}), got "
                                 f"{tuple(x.shape)}")
            src, stride, choff, by_view = x, x.shape[1] * HW, (x.shape[1] - 6) * HW, 1
        else:
            if tuple(y_t.shape) != (B, 3, H, W):
                raise ValueError(f"y_t must have shape {(B, 3, H, W)}, got {tuple(y_t.shape)}")
            src, stride = y_t, 3 * HW
    if keep is not None:
        keep = _drop_mask(keep, B, unet_out.device)
    x_hat = torch.empty(B, 3, H, W, device=unet_out.device, dtype=torch.float32)
    _call("vf_self_cond_estimate", _ptr(unet_out), ctypes.c_void_p(off.data_ptr()), _ptr(level), _ptr(src), stride, choff,
          by_view, None if keep is None else ctypes.c_void_p(keep.data_ptr()), _ptr(x_hat), B, Cout, HW, int(weighting),
          PREDICTIONS[prediction], _stream())
    return x_hat


# ---- the variational bound in bits per dimension (csrc/diffusion.hip holds the definition) ----
RNG_NLL_NOISE = 6                                                  # the kind of a noisy target's draw (csrc/rng.h)
NLL_TABLE_NAMES = ("a", "b", "c0", "hi", "lo")


def nll_scratch(B, device):
    """What nll_terms / nll_prior keep between their two launches: the per-(sample, chunk) partial sums."""
    return {"vb": torch.empty(B * 64, device=device, dtype=torch.float32),
            "sq": torch.empty(B * 64, device=device, dtype=torch.float32)}


def nll_noisy(y_0, kidx, tau, gammas, noise=None, seed=None, ids=None, out=None):
    """The noisy targets of step k = kidx[b] of the chain tau (device int64 (K,)) on the fp32 `gammas` buffer:
    y_k = sqrt(g) y_0 + sqrt(1 - g) n, g = gammas[tau[k]].  noise (B, K, 3, H, W) wins; else n is drawn in the kernel from
    (seed, ids[b], kind 6, tau[k], element).  One launch; with out= no allocation."""
    _check(y_0, gammas, noise, out)
    B, _, H, W = y_0.shape
    K = tau.numel()
    _check_i64("kidx", kidx, B)
    _check_i64("tau", tau, K)
    if noise is None and seed is None:
        raise ValueError("nll_noisy needs noise= or seed=")
    if noise is not None and tuple(noise.shape) != (B, K, 3, H, W):
        raise ValueError(f"noise must have shape {(B, K, 3, H, W)}, got {tuple(noise.shape)}")
    if out is None:
        out = torch.empty_like(y_0)
    elif tuple(out.shape) != tuple(y_0.shape):
        raise ValueError(f"out must have y_0's shape {tuple(y_0.shape)}, got {tuple(out.shape)}")
    sd, idp = 0, None
    if noise is None:
        ids = sample_ids(y_0.device, B, ids)
        _check_ids(ids, B)
        sd, idp = _seed(seed), ctypes.c_void_p(ids.data_ptr())
    _call("vf_nll_noisy", _ptr(y_0), _ptr(noise), sd, idp, ctypes.c_void_p(kidx.data_ptr()),
          ctypes.c_void_p(tau.data_ptr()), _ptr(gammas), _ptr(out), B, H * W, K, gammas.numel(), _stream())
    return out


def nll_terms(unet_out, off, y_k, y_0, kidx, tables, B, weighting, learned=False, decoder=False, large=False, clip=True,
              out=None, scratch=None):
    """One term of the bound for every sample at step k = kidx[b] (device int64 (B,)): column k of vb (B, K), the term in
    bits per dimension, and of x0_mse (B, K), the mean of (y0 - y_0)^2.  tables: the fp32 device tables a, b, c0, hi, lo
    (K,) of schedule.nll_tables.  learned: a nine-channel unet_out whose composed channels 6..8 place lp between lo[k] and
    hi[k]; else lp = hi[k] where large, lo[k] otherwise.  decoder: the discretised likelihood (the caller's k == 0)
    instead of the KL.  out=(vb, x0_mse) and scratch=nll_scratch(B, device): no allocation.  Two launches."""
    tabs = [tables[n] for n in NLL_TABLE_NAMES]
    _check(unet_out, y_k, y_0, *tabs)
    K = tabs[0].numel()
    if any(t.numel() != K for t in tabs) or K < 1:
        raise ValueError(f"nll_terms needs a, b, c0, hi and lo of one length, got {[t.numel() for t in tabs]}")
    if learned:
        _check_nine("nll_terms(learned=True)", unet_out)
        if large:
            raise ValueError("fixed_variance='large' on a learned variance: the model has its own")
    _, Cout, H, W = unet_out.shape
    if tuple(y_k.shape) != (B, 3, H, W) or tuple(y_0.shape) != (B, 3, H, W):
        raise ValueError(f"nll_terms needs y_k and y_0 of shape {(B, 3, H, W)}")
    _check_i64("kidx", kidx, B)
    if out is None:
        out = (torch.zeros(B, K, device=y_0.device, dtype=torch.float32),
               torch.zeros(B, K, device=y_0.device, dtype=torch.float32))
    vb, mse = out
    _check(vb, mse)
    if tuple(vb.shape) != (B, K) or tuple(mse.shape) != (B, K):
        raise ValueError(f"out= needs two tensors of shape {(B, K)}")
    if scratch is None:
        scratch = nll_scratch(B, y_0.device)
    if scratch["vb"].numel() < B * 64 or scratch["sq"].numel() < B * 64:
        raise ValueError(f"scratch= holds fewer than {B * 64} partial sums")
    _call("vf_nll_terms", _ptr(unet_out), ctypes.c_void_p(off.data_ptr()), _ptr(y_k), _ptr(y_0),
          ctypes.c_void_p(kidx.data_ptr()), *(_ptr(t) for t in tabs), _ptr(scratch["vb"]), _ptr(scratch["sq"]), _ptr(vb),
          _ptr(mse), B, Cout, H * W, K, int(bool(weighting)), int(bool(clip)), int(bool(learned)), int(bool(decoder)),
          int(bool(large)), _stream())
    return vb, mse


def nll_prior(y_0, gammas, out=None, scratch=None):
    """The prior term L_T of every sample, (B,) in bits per dimension: the KL of q(y_T | y_0) from N(0, I) at
    gammas[T - 1]; exactly 0 on a zero-terminal-SNR schedule.  out= and scratch=: no allocation.  Two launches."""
    _check(y_0, gammas, out)
    B, _, H, W = y_0.shape
    if out is None:
        out = torch.empty(B, device=y_0.device, dtype=torch.float32)
    elif out.numel() != B:
        raise ValueError(f"out= needs {B} elements")
    if scratch is None:
        scratch = nll_scratch(B, y_0.device)
    if scratch["vb"].numel() < B * 64:
        raise ValueError(f"scratch= holds fewer than {B * 64} partial sums")
    _call("vf_nll_prior", _ptr(y_0), _ptr(gammas), _ptr(scratch["vb"]), _ptr(out), B, H * W, gammas.numel(), _stream())
    return out


def nll_terms_host(out, o, y_k, y_0, a, b, c0, hi, lo, learned=False, decoder=False, large=False, clip=True):
    """The host mirror of one term of the bound: float tensors / sequences of one length (o: None unless learned) ->
    (term in bits, (y0 - y_0)^2) float32 CPU tensors, per element, by the function the kernel runs.  No GPU."""
    names = (out, y_k, y_0, a, b, c0, hi, lo) + ((o,) if learned else ())
    arrs = [torch.as_tensor(v, dtype=torch.float32).detach().cpu().reshape(-1).contiguous() for v in names]
    n = arrs[0].numel()
    if any(v.numel() != n for v in arrs):
        raise ValueError("nll_terms_host needs inputs of one length")
    outs = [torch.empty(n, dtype=torch.float32) for _ in range(2)]
    p = lambda v: ctypes.c_void_p(v.data_ptr())                     # noqa: E731
    rc = _lib.load().vf_nll_terms_host(p(arrs[0]), p(arrs[8]) if learned else None, *(p(v) for v in arrs[1:8]),
                                       int(bool(learned)), int(bool(decoder)), int(bool(large)), int(bool(clip)),
                                       p(outs[0]), p(outs[1]), n)
    if rc != 0:
        raise _lib.VFHipError(f"vf_nll_terms_host failed with {rc}")
    return tuple(outs)


# ---- the analytic variance: the second moment of the noise estimate (csrc/diffusion.hip holds the definition) ----
EPS_TABLE_NAMES = ("ea", "eb")


def eps_moments(unet_out, off, y_k, kidx, tables, B, weighting, out=None, scratch=None):
    """The second moment of the noise estimate of every sample at step k = kidx[b] (device int64 (B,)): column k of
    m2 (B, K), the mean over the sample's 3 H W elements of (ea[k] y_k + eb[k] out_b)^2 with out_b the composition of
    channels 0..2 over the sample's views (channels 6..8 of a nine-channel output are ignored).  tables: the fp32 device
    tables ea, eb (K,) of schedule.eps_tables.  out=(B, K) and scratch=nll_scratch(B, device): no allocation; only
    column k is written.  Two launches."""
    tabs = [tables[n] for n in EPS_TABLE_NAMES]
    _check(unet_out, y_k, *tabs)
    K = tabs[0].numel()
    if tabs[1].numel() != K or K < 1:
        raise ValueError(f"eps_moments needs ea and eb of one length, got {[t.numel() for t in tabs]}")
    _, Cout, H, W = unet_out.shape
    if tuple(y_k.shape) != (B, 3, H, W):
        raise ValueError(f"eps_moments needs y_k of shape {(B, 3, H, W)}, got {tuple(y_k.shape)}")
    _check_i64("kidx", kidx, B)
    if out is None:
        out = torch.zeros(B, K, device=y_k.device, dtype=torch.float32)
    _check(out)
    if tuple(out.shape) != (B, K):
        raise ValueError(f"out= needs a tensor of shape {(B, K)}")
    if scratch is None:
        scratch = nll_scratch(B, y_k.device)
    if scratch["vb"].numel() < B * 64:
        raise ValueError(f"scratch= holds fewer than {B * 64} partial sums")
    _call("vf_eps_moments", _ptr(unet_out), ctypes.c_void_p(off.data_ptr()), _ptr(y_k), ctypes.c_void_p(kidx.data_ptr()),
          _ptr(tabs[0]), _ptr(tabs[1]), _ptr(scratch["vb"]), _ptr(out), B, Cout, H * W, K, int(bool(weighting)),
          _stream())
    return out


def eps_moment_host(out, y_k, ea, eb):
    """The host mirror of one element of the moment: float tensors / sequences of one length -> (the noise estimate
    ea y_k + eb out, its square) float32 CPU tensors, per element, by the function the kernel runs.  No GPU."""
    arrs = [torch.as_tensor(v, dtype=torch.float32).detach().cpu().reshape(-1).contiguous() for v in (out, y_k, ea, eb)]
    n = arrs[0].numel()
    if any(v.numel() != n for v in arrs):
        raise ValueError("eps_moment_host needs inputs of one length")
    outs = [torch.empty(n, dtype=torch.float32) for _ in range(2)]
    p = lambda v: ctypes.c_void_p(v.data_ptr())                     # noqa: E731
    rc = _lib.load().vf_eps_moment_host(*(p(v) for v in arrs), p(outs[0]), p(outs[1]), n)
    if rc != 0:
        raise _lib.VFHipError(f"vf_eps_moment_host failed with {rc}")
    return tuple(outs)


def psnr(generated, target):
    """Per-image PSNR (B,) of (B,C,H,W) tensors in [0,1]."""
    generated, target = _c(generated), _c(target)
    _check(generated, target)
    B = generated.shape[0]
    out = torch.empty(B, device=generated.device, dtype=torch.float32)
    _call("vf_psnr", _ptr(generated), _ptr(target), _ptr(out), B, generated[0].numel(), _stream())
    return out


SSIM_WIN, SSIM_SIGMA = 11, 1.5


def _ssim_window(device):
    """The normalised 11-tap Gaussian of pytorch_msssim (`_fspecial_gauss_1d`), built with the same fp32 torch
    operations on the host and kept on the device.  The first call per device copies it there, so it must not be a
    call inside a graph capture."""
    win = st._SSIM_WINDOW.get(device)
    if win is None:
        coords = torch.arange(SSIM_WIN, dtype=torch.float32)
        coords -= SSIM_WIN // 2
        g = torch.exp(-(coords ** 2) / (2 * SSIM_SIGMA ** 2))
        g /= g.sum()
        win = st._SSIM_WINDOW[device] = g.to(device)
    return win


def ssim(generated, target, data_range=1.0):
    """Per-image SSIM (B,) of (B,C,H,W) tensors: pytorch_msssim.ssim(generated, target, data_range,
    size_average=False) with its defaults, H, W >= 11 (the package skips the smoothing along a shorter side; that
    quantity is not SSIM and is refused here)."""
    if generated.dim() != 4 or generated.shape != target.shape:
        raise ValueError(f"ssim needs two (B,C,H,W) tensors of one shape, got {tuple(generated.shape)} and "
                         f"{tuple(target.shape)}")
    B, C, H, W = generated.shape
    if H < SSIM_WIN or W < SSIM_WIN or C < 1:
        raise ValueError(f"ssim needs at least one channel and H, W >= {SSIM_WIN} (the window), got "
                         f"{tuple(generated.shape)}")
    generated, target = _c(generated), _c(target)
    _check(generated, target)
    out = torch.empty(B, device=generated.device, dtype=torch.float32)
    if B == 0:
        return out
    ws = _workspace(generated.device, _lib.load().vf_ssim_workspace_floats(B, C, H, W))
    _call("vf_ssim", _ptr(generated), _ptr(target), _ptr(out), _ptr(ws), B, C, H, W,
          _ptr(_ssim_window(generated.device)), float(data_range), _stream())
    return out
