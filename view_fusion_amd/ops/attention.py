"""Self-attention core (reference model/unet.py:258-277) and the channel concatenation fallback."""
import math

import torch

from .state import st
from .core import _c, _call, _check, _launch, _ptr, _stream
from .dense import _bgemm


# ---------------------------------------------------------------------------------------------
# VF_ATTN_DSCORE=0: tuning aid -- the attention backward's dP product + softmax backward as two launches (rounds 1-4)


class _AttentionFn(torch.autograd.Function):
    """softmax(Q^T K / sqrt(C)) applied to V for single-head spatial attention; qkv (S,3C,H,W)."""

    @staticmethod
    def forward(ctx, qkv, need_p):
        _check(qkv)
        S, C3, H, W = qkv.shape
        C, L = C3 // 3, H * W
        alpha = 1.0 / math.sqrt(C)
        out = torch.empty(S, C, H, W, device=qkv.device, dtype=torch.float32)
        if L in (64, 256) and C % 32 == 0:        # fused flash-style kernel, scores stay in registers
            P = torch.empty(S, L, L, device=qkv.device, dtype=torch.float32) if need_p else None
            _launch("attn_fwd", 4.0 * S * L * L * C, "vf_attention_fwd", _ptr(qkv), _ptr(out), _ptr(P), S, C, L, _stream(),
                    nbytes=4.0 * (qkv.numel() + out.numel() + (S * L * L if need_p else 0)))
        else:                                     # generic sizes: materialised scores
            P = torch.empty(S, L, L, device=qkv.device, dtype=torch.float32)
            _bgemm(qkv, qkv, P, None, S, L, L, C, (C3 * L, 1, L), (C3 * L, L, 1), (L * L, L, 1), alpha,
                   offA=0, offB=C * L)
            _call("vf_softmax_fwd", _ptr(P), _ptr(P), S * L, L, _stream())
            _bgemm(qkv, P, out, None, S, C, L, L, (C3 * L, L, 1), (L * L, 1, L), (C * L, L, 1), offA=2 * C * L)
        ctx.save_for_backward(qkv, P)
        return out

    @staticmethod
    def backward(ctx, dO):
        qkv, P = ctx.saved_tensors
        dO = _c(dO)
        S, C3, H, W = qkv.shape
        C, L = C3 // 3, H * W
        alpha = 1.0 / math.sqrt(C)
        dqkv = torch.empty_like(qkv)
        dS = torch.empty_like(P)
        st._KIND_OVERRIDE = "attn_bwd" if st.KERNEL_LOG is not None else None
        fused_dq, fused_dvdk = attention_bwd_route(C, L)
        if fused_dq:
            # one launch (round 5): dS = P o (dP - rowsum(P o dP)) with dP[i][j] = sum_c dO[c][i] v[c][j] never written,
            # and dQ[c][i] = alpha sum_j k[c][j] dS[i][j] from the dS values still in registers
            _call("vf_attention_dscore", _ptr(qkv), _ptr(dO), _ptr(P), _ptr(dS), _ptr(dqkv), S, C, L, _stream(),
                  flops=4.0 * S * L * L * C)
        else:
            # dP[i][j] = sum_c dO[c][i] v[c][j]
            _bgemm(dO, qkv, dS, None, S, L, L, C, (C * L, 1, L), (C3 * L, L, 1), (L * L, L, 1), offB=2 * C * L)
            _call("vf_softmax_bwd", _ptr(P), _ptr(dS), _ptr(dS), S * L, L, _stream())
        if fused_dvdk:
            # dV and dK (below) in one launch of a kernel written for these two products (round 5)
            _call("vf_attention_dvdk", _ptr(qkv), _ptr(dO), _ptr(P), _ptr(dS), _ptr(dqkv), S, C, L, _stream(),
                  flops=4.0 * S * L * L * C)
            st._KIND_OVERRIDE = None
            return dqkv, None
        # dV[c][j] = sum_i dO[c][i] P[i][j]
        _bgemm(dO, P, dqkv, None, S, C, L, L, (C * L, L, 1), (L * L, L, 1), (C3 * L, L, 1), offC=2 * C * L)
        if not fused_dq:
            # dQ[c][i] = alpha sum_j k[c][j] dS[i][j]
            _bgemm(qkv, dS, dqkv, None, S, C, L, L, (C3 * L, L, 1), (L * L, 1, L), (C3 * L, L, 1), alpha,
                   offA=C * L, offC=0)
        # dK[c][j] = alpha sum_i q[c][i] dS[i][j]
        _bgemm(qkv, dS, dqkv, None, S, C, L, L, (C3 * L, L, 1), (L * L, L, 1), (C3 * L, L, 1), alpha,
               offA=0, offC=C * L)
        st._KIND_OVERRIDE = None
        return dqkv, None


STREAM_MIN_L = 4097          # maps of more pixels take the streaming kernels: the materialised P would not fit


def attention_route(C, L):
    """Which kernels ops.attention runs for a (C, L) map: "fused" (L = 64 / 256, C % 32 == 0, scores in registers),
    "generic" (the materialised S x L x L scores, L <= 4096) or "stream" (csrc/attention_stream.hip, L > 4096)."""
    if L >= STREAM_MIN_L:
        return "stream"
    if L in (64, 256) and C % 32 == 0:
        return "fused"
    return "generic"


def attention_bwd_route(C, L):
    """(dscore, dvdk): whether _AttentionFn.backward runs vf_attention_dscore (dS + dQ in one launch) and
    vf_attention_dvdk (dV + dK in one launch) at a (C, L) map; every product a kernel does not take is a vf_bgemm call, and
    without dscore the softmax backward is a launch of its own.  The library states the same route (vf_attention_bwd_plan);
    tests/test_attn_plan_host.py holds the two together."""
    dscore = L == 256 and C % 32 == 0 and bool(st.ATTN_DSCORE)
    return dscore, dscore and C % 64 == 0 and bool(st.ATTN_DVDK)


class _AttentionStreamFn(torch.autograd.Function):
    """The same attention without any L x L buffer (csrc/attention_stream.hip): online softmax over key blocks, the
    backward recomputes the probabilities from the saved per-query (scaled maximum, 1 / sum).  Training saves (qkv, out,
    rowstat)."""

    @staticmethod
    def forward(ctx, qkv, need_stat):
        _check(qkv)
        S, C3, H, W = qkv.shape
        C, L = C3 // 3, H * W
        out = torch.empty(S, C, H, W, device=qkv.device, dtype=torch.float32)
        rowstat = torch.empty(S, 2, L, device=qkv.device, dtype=torch.float32) if need_stat else None
        _launch("attn_fwd", 4.0 * S * L * L * C, "vf_attn_stream_fwd", _ptr(qkv), _ptr(out), _ptr(rowstat), S, C, L,
                _stream(), nbytes=4.0 * (qkv.numel() + out.numel() + (2 * S * L if need_stat else 0)))
        ctx.save_for_backward(qkv, out, rowstat)
        return out

    @staticmethod
    def backward(ctx, dO):
        qkv, out, rowstat = ctx.saved_tensors
        dO = _c(dO)
        S, C3, H, W = qkv.shape
        C, L = C3 // 3, H * W
        dqkv = torch.empty_like(qkv)
        delta = torch.empty(S, L, device=qkv.device, dtype=torch.float32)
        # executed FLOPs: 8 L^2 C per view in the dK / dV kernel (S, dP, dV, dK) + 6 L^2 C in the dQ kernel (S and dP
        # recomputed, dQ)
        _launch("attn_bwd", 14.0 * S * L * L * C, "vf_attn_stream_bwd", _ptr(qkv), _ptr(out), _ptr(dO), _ptr(rowstat),
                _ptr(delta), _ptr(dqkv), S, C, L, _stream(),
                nbytes=4.0 * (2 * qkv.numel() + 2 * out.numel() + 3 * S * L))
        return dqkv, None


def attention_streaming(qkv):
    """Self-attention core on the streaming kernels at any L (O(L) memory); ops.attention routes L > 4096 here."""
    return _AttentionStreamFn.apply(qkv, torch.is_grad_enabled() and qkv.requires_grad)


def attention(qkv):
    if attention_route(qkv.shape[1] // 3, qkv.shape[2] * qkv.shape[3]) == "stream":
        return attention_streaming(qkv)
    return _AttentionFn.apply(qkv, torch.is_grad_enabled() and qkv.requires_grad)


class _ConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _check(a, b)
        S, Ca, H, W = a.shape
        Cb = b.shape[1]
        out = torch.empty(S, Ca + Cb, H, W, device=a.device, dtype=torch.float32)
        _call("vf_concat_channels", _ptr(a), _ptr(b), _ptr(out), S, Ca * H * W, Cb * H * W, 0, _stream())
        ctx.shapes = (a.shape, b.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = _c(dout)
        sa, sb = ctx.shapes
        da = torch.empty(sa, device=dout.device, dtype=torch.float32)
        db = torch.empty(sb, device=dout.device, dtype=torch.float32)
        _call("vf_concat_channels", _ptr(da), _ptr(db), _ptr(dout), sa[0], da[0].numel(), db[0].numel(), 1,
                  _stream())
        return da, db


def concat_channels(a, b):
    return _ConcatFn.apply(a, b)
