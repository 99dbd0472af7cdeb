"""Linear layers, the grouped FeatureWiseAffine launch, Swish, Dropout and the sin / cos embedding (reference
model/unet.py:27-32, 142-182)."""
import ctypes
import functools
import math

import torch

from .. import _lib, reducer
from .state import st
from .core import _c, _call, _check, _ptr, _stream
from .deferred import _gout


# ---------------------------------------------------------------------------------------------
def _bgemm(A, B, C, bias, batch, M, N, K, sA, sB, sC, alpha=1.0, beta=0.0, offA=0, offB=0, offC=0):
    _call("vf_bgemm", _ptr(A, offA), _ptr(B, offB), _ptr(C, offC), _ptr(bias), batch, M, N, K, sA[0], sA[1],
              sA[2], sB[0], sB[1], sB[2], sC[0], sC[1], sC[2], alpha, beta, _stream(), flops=2.0 * batch * M * N * K)


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        _check(x, w, b)
        S, I = x.shape
        O = w.shape[0]
        y = torch.empty(S, O, device=x.device, dtype=torch.float32)
        _bgemm(x, w, y, b, 1, S, O, I, (0, I, 1), (0, 1, I), (0, O, 1))
        ctx.save_for_backward(x, w)
        ctx.pw, ctx.pb = w, b
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _c(dy)
        S, I = x.shape
        O = w.shape[0]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _bgemm(dy, w, dx, None, 1, S, I, O, (0, O, 1), (0, I, 1), (0, I, 1))
        if ctx.needs_input_grad[1]:
            dw = _gout(ctx.pw, O, I, like=x)
            _bgemm(dy, x, dw, None, 1, O, I, S, (0, 1, O), (0, I, 1), (0, I, 1))
        if ctx.needs_input_grad[2]:
            db = _gout(ctx.pb, O, like=x)
            _call("vf_colsum", _ptr(dy), _ptr(db), 1, S, O, _stream())
        return dx, dw, db


def linear(x, weight, bias):
    """(S,I) @ weight(O,I)^T + bias -> (S,O)."""
    return _LinearFn.apply(x, weight, bias)


# ---------------------------------------------------------------------------------------------
# All FeatureWiseAffine linears of the UNet (30 x Linear(K -> C_g) on the SAME embedding) as one grouped launch.


def _ta_desc(layers, S, device):
    key = (S, device, tuple(l.weight.data_ptr() for l in layers), tuple(l.bias.data_ptr() for l in layers))
    hit = st._TA_DESC.get(id(layers[0]))
    if hit is not None and hit[0] == key:
        return hit[1]
    rows, coff = [], 0
    for l in layers:
        C = l.weight.shape[0]
        rows.append([l.weight.data_ptr(), l.bias.data_ptr(), C, S * coff, coff])
        coff += C
    plan = (torch.tensor(rows, dtype=torch.int64).to(device), [r[2] for r in rows], [r[4] for r in rows], coff)
    st._TA_DESC[id(layers[0])] = (key, plan)
    return plan


class _TimeAffineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, layers, *params):          # params = (w_0, b_0, w_1, b_1, ...) of `layers`, for autograd
        _check(emb, *params)
        S, K = emb.shape
        desc, Cs, coffs, CT = _ta_desc(layers, S, emb.device)
        out = torch.empty(S * CT, device=emb.device, dtype=torch.float32)
        _call("vf_time_affine_fwd", ctypes.c_void_p(desc.data_ptr()), len(Cs), _ptr(emb), _ptr(out), S, K, CT,
                  _stream())
        ctx.save_for_backward(emb)
        ctx.plan = (desc, Cs, coffs, CT)
        ctx.params = params
        return tuple(out[S * o:S * (o + C)].view(S, C) for C, o in zip(Cs, coffs))

    @staticmethod
    def backward(ctx, *grads):
        (emb,) = ctx.saved_tensors
        desc, Cs, coffs, CT = ctx.plan
        S, K = emb.shape
        de = torch.cat([(g if g is not None else emb.new_zeros(S, C)).reshape(-1) for g, C in zip(grads, Cs)])
        slots = gdst = dw = db = None
        arena = reducer.ACTIVE
        if arena is not None:                       # every layer's dW / db straight into its arena slot
            slots = [arena.slot(p) for p in ctx.params]
            if any(t is None for t in slots):
                slots = None
            else:
                # (keyed on the slots, not on the parameter objects: a captured step runs on leaf aliases of the
                # parameters and must find the table the eager iterations before it uploaded -- no copy in a capture)
                key = (id(arena), arena.base, slots[0].data_ptr(), len(slots))
                hit = st._TA_GDST.get(key)
                if hit is None:
                    rows = [[slots[2 * g].data_ptr(), slots[2 * g + 1].data_ptr()] for g in range(len(Cs))]
                    hit = (key, torch.tensor(rows, dtype=torch.int64).to(emb.device))
                    if len(st._TA_GDST) > 8:
                        st._TA_GDST.clear()
                    st._TA_GDST[key] = hit
                gdst = hit[1]
        if slots is None:
            dw = torch.empty(CT, K, device=emb.device, dtype=torch.float32)
            db = torch.empty(CT, device=emb.device, dtype=torch.float32)
        demb = ws = None
        if ctx.needs_input_grad[0]:
            demb = torch.empty_like(emb)
            ws = torch.empty(_lib.load().vf_time_affine_ws_floats(S, K), device=emb.device, dtype=torch.float32)
        _call("vf_time_affine_bwd", ctypes.c_void_p(desc.data_ptr()), len(Cs), _ptr(emb), _ptr(de), _ptr(dw),
                  _ptr(db), ctypes.c_void_p(gdst.data_ptr()) if gdst is not None else None, _ptr(demb), _ptr(ws), S, K,
                  CT, _stream())
        out = [demb, None]
        if slots is not None:
            return tuple(out + slots)
        for C, o in zip(Cs, coffs):
            out += [dw[o:o + C], db[o:o + C]]
        return tuple(out)


def time_affine_all(emb, layers):
    """[Linear_g(emb) for g in layers] (each (S, C_g)) in one launch; `layers` = list of nn.Linear holders."""
    params = []
    for l in layers:
        params += [l.weight, l.bias]
    return _TimeAffineFn.apply(emb, layers, *params)


class _SwishFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _check(x)
        y = torch.empty_like(x)
        _call("vf_swish_fwd", _ptr(x), _ptr(y), x.numel(), _stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _c(dy)
        dx = torch.empty_like(x)
        _call("vf_swish_bwd", _ptr(x), _ptr(dy), _ptr(dx), x.numel(), _stream())
        return dx


def swish(x):
    return _SwishFn.apply(x)


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, u, p):
        _check(x, u)
        y = torch.empty_like(x)
        _call("vf_dropout", _ptr(x), _ptr(u), _ptr(y), x.numel(), float(p), _stream())
        ctx.save_for_backward(u)
        ctx.p = float(p)
        return y

    @staticmethod
    def backward(ctx, dy):
        (u,) = ctx.saved_tensors
        dy = _c(dy)
        dx = torch.empty_like(dy)
        _call("vf_dropout", _ptr(dy), _ptr(u), _ptr(dx), dy.numel(), ctx.p, _stream())
        return dx, None, None


def dropout(x, p, u=None):
    """nn.Dropout(p) in training mode (reference Block, unet.py:207-216): x * (u >= p) / (1 - p).  u = uniform draws
    in [0,1) shaped like x (default: torch's device RNG; tests inject them)."""
    if u is None:
        u = torch.rand_like(x)
    return _DropoutFn.apply(x, _c(u), p)


_DROPOUT_MAX_VIEWS, _DROPOUT_MAX_LAYERS = (1 << 12) - 1, 1 << 16     # csrc/rng.h, kind 5: step = (layer << 12) | view


@functools.lru_cache(maxsize=16)
def dropout_constants(p):
    """(thr, scale) of the seeded Dropout (csrc/rng.h, "Dropout masks"): thr = ceil(float32(p) * 2^24), the product
    exact in double precision, and scale = 1.0f / (1.0f - p) evaluated in fp32 as vf_dropout does."""
    p32 = torch.tensor(float(p), dtype=torch.float32)
    if not 0.0 <= float(p32) < 1.0:                  # (also refuses NaN)
        raise ValueError(f"dropout probability has to be in [0, 1), got {p}")
    return int(math.ceil(float(p32) * 2.0 ** 24)), float(1.0 / (1.0 - p32))


class _DropoutSeededFn(torch.autograd.Function):
    """Dropout whose mask is drawn in the kernel: nothing but ids and off (a few hundred bytes) is saved, and the
    backward is the same launch on dy."""

    @staticmethod
    def forward(ctx, x, seed, ids, off, thr, scale, layer):
        ctx.save_for_backward(ids, off)
        ctx.args = (seed, thr, scale, layer)
        return _dropout_seeded_launch(x, seed, ids, off, thr, scale, layer)

    @staticmethod
    def backward(ctx, dy):
        ids, off = ctx.saved_tensors
        seed, thr, scale, layer = ctx.args
        return _dropout_seeded_launch(_c(dy), seed, ids, off, thr, scale, layer), None, None, None, None, None, None


def _dropout_seeded_launch(x, seed, ids, off, thr, scale, layer):
    y = torch.empty_like(x)
    S = x.shape[0]
    _call("vf_dropout_seeded", _ptr(x), _ptr(y), seed, ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(off.data_ptr()),
          ids.numel(), S, x.numel() // S, thr, scale, layer, _stream())
    return y


def dropout_seeded(x, p, seed, ids, off, layer, max_views=None):
    """nn.Dropout(p) in training mode with the mask drawn inside the kernel from the counter-based generator
    (csrc/rng.h, kind 5): a pure function of (seed, sample id, view index, layer, element), so it does not depend on the
    row a sample occupies, on the rest of the batch or on the rank.  Bit-identical to dropout(x, p, u) with
    u = (word >> 8) * 2^-24; no u exists, forward or saved.
    x (S, ...): one row per view; ids: device int64 (B,) (ops.sample_ids); off: device int32 (B + 1,) (ops.view_offsets),
    off[B] == S.  max_views: the largest view count when the caller knows it on the host (view_offsets' third result).
    ValueError, before any launch, for a sample with more than 4095 views or layer outside [0, 65536)."""
    _check(x)
    layer = int(layer)
    if not 0 <= layer < _DROPOUT_MAX_LAYERS:
        raise ValueError(f"a seeded Dropout layer index must be in [0, {_DROPOUT_MAX_LAYERS}), got {layer}")
    B, S = ids.numel(), x.shape[0]
    if (not ids.is_cuda or ids.dtype != torch.int64 or not ids.is_contiguous() or not off.is_cuda
            or off.dtype != torch.int32 or not off.is_contiguous() or off.numel() != B + 1):
        raise _lib.VFHipError(f"seeded Dropout needs device int64 ids (B,) and device int32 off (B + 1,), B = {B}")
    if max_views is None and S > _DROPOUT_MAX_VIEWS:
        # only a batch of more than 4095 rows can hold such a sample: the counts are read back in that case alone
        host = off.cpu()
        max_views = int((host[1:] - host[:-1]).max())
    if max_views is not None and max_views > _DROPOUT_MAX_VIEWS:
        raise ValueError(f"seeded Dropout numbers a sample's views in 12 bits: {max_views} views exceed "
                         f"{_DROPOUT_MAX_VIEWS}")
    if S == 0 or x.numel() == 0:
        return x
    if (x.numel() // S) % 4:
        raise ValueError(f"seeded Dropout draws four elements per call: a row of {x.numel() // S} elements is no "
                         f"multiple of 4")
    thr, scale = dropout_constants(p)
    return _DropoutSeededFn.apply(x, int(seed) & 0xFFFFFFFFFFFFFFFF, ids, off, thr, scale, layer)


def sincos_embedding(level, angle, dim):
    """(S,1),(S,1) -> (S,dim): [sin|cos](level*f) ++ [sin|cos](angle*f), dim/4 frequencies."""
    level = _c(level.detach().reshape(-1).float())
    angle = _c(angle.detach().reshape(-1).float())
    _check(level, angle)
    S = level.numel()
    out = torch.empty(S, dim, device=level.device, dtype=torch.float32)
    _call("vf_sincos_embed", _ptr(level), _ptr(angle), _ptr(out), S, dim, _stream())
    return out
