"""Conditioning cases for the softmax / normalisation kernels: seeded hard inputs, float64 restatements, the same
operations in stock fp32 torch on the CPU, and the one comparison rule (the convention of tests/ssim_ref.py, rng_ref.py,
lpips_ref.py):

    err(a) = max|a - r64| / max|r64|;   e = err(stock fp32 CPU) on THIS case's inputs;
    a kernel passes if err <= max(4 e, tol), tol = the family's stated tolerance (TOL below), any non-finite value fails.

Every case must have e <= CAP = 2.5e-4 (so no bound exceeds 1e-3): a case above it is an error of the case list
(`bound` asserts), never a skip.  Imports no GPU code."""
import math

import torch
import torch.nn.functional as F

CAP = 2.5e-4          # the largest fp32-restatement error a case may have
MARGIN = 4.0          # another equally legitimate fp32 evaluation order (ssim_ref.bound)
EPS = 1e-5            # nn.GroupNorm's eps everywhere in the UNet

# The families' stated tolerances (tests/test_gpu_kernels.py: docstring, test_group_norm_fwd_bwd, test_attention_fwd_bwd,
# test_winograd_fixup_evaluates_the_groupnorm, test_conv_small_groupnorm_without_a_launch, test_compose_loss_and_stack,
# test_p_sample_tail; DESIGN 5 "kernels rel 2e-5").
TOL = {"gn_fwd": 1e-5, "gn_bwd": 2e-5, "attn_fwd": 2e-5, "attn_bwd": 5e-5, "conv_gn": 2e-5, "small_h": 2e-6,
       "small_y": 5e-6, "compose": 1e-5, "compose_loss": 1e-6, "softmax": 9e-7}

# "softmax" (vf_softmax_fwd / _bwd alone, no stated tolerance): four times the largest stock fp32 error over
# attn_plan_ref.softmax_cases(), rounded up to one digit (2.04e-7 -> 9e-7; tests/test_attn_plan_host.py recomputes it).

# The grid (ISSUE: fp32 CPU e <= 7.2e-5 for GroupNorm at ratio 100, 1.1e-3 at ratio 1000 -- not used; attention scale 14:
# e <= 6.9e-5).  Compose logit scales chosen the same way: e (measured on the CPU, test_cond_host) stays below 1e-6 up to
# 100, and exp(100) overflows fp32, so a softmax without its maximum cannot pass.
GN_RATIOS, GN_SIGMAS = (0, 10, 100), (1e-3, 1.0, 1e3)
ATTN_SCALES, ATTN_SHIFTS = (2, 6, 14), (0, 8)
COMPOSE_SCALES = (4, 30, 100)
CONST_C = 0.75        # the constant group's value: exactly representable in fp32


def _u(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1


# ------------------------------------------------------------------------------------------------ the rule
def err(a, r64):
    """max|a - r64| / max|r64|; inf where a holds a non-finite value."""
    a, r64 = a.detach().double().cpu(), r64.detach().double().cpu()
    if not bool(torch.isfinite(a).all()):
        return float("inf")
    return float((a - r64).abs().max() / r64.abs().max().clamp_min(1e-30))


def bound(e, tol, extra=0.0):
    """max(4 e, tol + extra); `extra` is only ever the derived constant-group term."""
    assert e <= CAP, f"case list error: the fp32 restatement's own error {e:.3e} exceeds the cap {CAP:.1e}"
    return max(MARGIN * e, tol + extra)


def judge(a, r64, r32, tol, extra=0.0):
    """-> (err of a, e, bound, passes)."""
    e = err(r32, r64)
    b = bound(e, tol, extra)
    d = err(a, r64)
    return d, e, b, d <= b


# ------------------------------------------------------------------------------------------------ GroupNorm
def gn_input(S, C, H, W, ratio, sigma, seed, variant=None, groups=32):
    """x = sigma u + a per-(view, group) offset drawn in +-ratio sigma (u uniform in (-1, 1)), float32.
    variant "const": group 1 of view 0 is exactly CONST_C;  "outlier": one pixel of view S-1 at 1e4 sigma."""
    cpg = C // groups
    x = sigma * _u((S, C, H, W), seed)
    off = ratio * sigma * _u((S, groups), seed + 1)
    x = x + off.repeat_interleave(cpg, dim=1)[:, :, None, None]
    if variant == "const":
        x[0, cpg:2 * cpg] = CONST_C
    elif variant == "outlier":
        x[S - 1, C - 1, H // 2, W // 3] = 1e4 * sigma
    else:
        assert variant is None
    return x.float()


def gn_params(S, C, H, W, seed):
    """gamma, beta, dy (float32)."""
    return (1 + 0.2 * _u((C,), seed + 2)).float(), (0.2 * _u((C,), seed + 3)).float(), _u((S, C, H, W), seed + 4).float()


def gn_forward_f64(x, gamma, beta, silu, groups=32):
    """Two-pass GroupNorm(+Swish) restated in float64 (biased variance, eps inside the root)."""
    S, C, H, W = x.shape
    xg = x.double().reshape(S, groups, -1)
    mean = xg.mean(-1, keepdim=True)
    var = ((xg - mean) ** 2).mean(-1, keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + EPS)).reshape(S, C, H, W) * gamma.double()[None, :, None, None] \
        + beta.double()[None, :, None, None]
    return y * torch.sigmoid(y) if silu else y


def _grads(fn, inputs, dy):
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    y = fn(*leaves)
    y.backward(dy.to(y.dtype))
    return [y.detach()] + [t.grad for t in leaves]


def gn_ref(x, gamma, beta, dy, silu, groups=32):
    """-> (r64, r32): each [y, dx, dgamma, dbeta]; r64 from the float64 restatement, r32 from stock F.group_norm."""
    r64 = _grads(lambda a, g, b: gn_forward_f64(a, g, b, silu, groups), (x.double(), gamma.double(), beta.double()), dy)

    def f32(a, g, b):
        y = F.group_norm(a, groups, g, b, EPS)
        return y * torch.sigmoid(y) if silu else y
    return r64, _grads(f32, (x, gamma, beta), dy)


def const_group_term(gamma):
    """A mean one ulp off (sum * inv_n) moves a constant group's output by at most ulp32(c) |gamma|max / sqrt(eps)."""
    ulp = 2.0 ** (math.floor(math.log2(CONST_C)) - 23)
    return ulp * float(gamma.abs().max()) / math.sqrt(EPS)


def act(v, silu):
    v = v.double()
    return v * torch.sigmoid(v) if silu else v


# ------------------------------------------------------------------------------------------------ GroupNorm behind a conv
def conv_gn_case(S, Cin, Cout, H, ratio, seed=41):
    """conv (bias + per-view bias + residual) -> GroupNorm(32) + Swish whose group offset comes from the conv bias:
    bias = ratio sigma_out per group, sigma_out the standard deviation of the bias-free conv output.
    -> (conv, gn, x, vb, res, r64, r32), each reference [y, gn(y)]."""
    conv, gn = torch.nn.Conv2d(Cin, Cout, 3, padding=1), torch.nn.GroupNorm(32, Cout)
    x, vb = _u((S, Cin, H, H), seed).float(), 0.3 * _u((S, Cout), seed + 1).float()
    res = 0.5 * _u((S, Cout, H, H), seed + 2).float()
    with torch.no_grad():
        conv.weight.copy_(_u((Cout, Cin, 3, 3), seed + 3) / math.sqrt(Cin * 9))
        sigma_out = float(F.conv2d(x.double(), conv.weight.double(), padding=1).std())
        conv.bias.copy_((ratio * sigma_out * _u((32,), seed + 4)).repeat_interleave(Cout // 32))
        gn.weight.copy_(1 + 0.3 * _u((Cout,), seed + 5))
        gn.bias.copy_(0.2 * _u((Cout,), seed + 6))

    def ref(dt):
        y = F.conv2d(x.to(dt), conv.weight.to(dt), conv.bias.to(dt), padding=1) + vb.to(dt)[:, :, None, None] + res.to(dt)
        a = gn_forward_f64(y, gn.weight, gn.bias, True) if dt == torch.float64 else \
            F.silu(F.group_norm(y, 32, gn.weight, gn.bias, EPS))
        return [y.detach(), a.detach()]
    return conv, gn, x, vb, res, ref(torch.float64), ref(torch.float32)


def conv_small_case(C0, C1, C2, H, KS2, ratio, S=2):
    """conv 3x3 -> GroupNorm(32)[+Swish when the second conv is 3x3] -> conv KS2 x KS2; the first conv's bias puts the group
    mean at +-ratio standard deviations of its bias-free output.  -> (conv1, gn, conv2, x, silu, r64, r32), each
    reference [h (first conv's output), y]."""
    silu = KS2 == 3
    conv1, conv2 = torch.nn.Conv2d(C0, C1, 3, padding=1), torch.nn.Conv2d(C1, C2, KS2, padding=KS2 // 2)
    gn = torch.nn.GroupNorm(32, C1)
    x = _u((S, C0, H, H), 51).float()
    with torch.no_grad():
        conv1.weight.copy_(_u((C1, C0, 3, 3), 52) / math.sqrt(C0 * 9))
        sigma_out = float(F.conv2d(x.double(), conv1.weight.double(), padding=1).std())
        sign = torch.where(torch.arange(32) % 2 == 0, 1.0, -1.0).double()
        conv1.bias.copy_((ratio * sigma_out * sign).repeat_interleave(C1 // 32))
        conv2.weight.copy_(_u((C2, C1, KS2, KS2), 54) / math.sqrt(C1 * KS2 * KS2))
        conv2.bias.copy_(0.1 * _u((C2,), 55))
        gn.weight.copy_(1 + 0.3 * _u((C1,), 56))
        gn.bias.copy_(0.2 * _u((C1,), 57))

    def ref(dt):
        h = F.conv2d(x.to(dt), conv1.weight.to(dt), conv1.bias.to(dt), padding=1)
        if dt == torch.float64:
            n = gn_forward_f64(h, gn.weight, gn.bias, silu)
        else:
            n = F.group_norm(h, 32, gn.weight, gn.bias, EPS)
            n = F.silu(n) if silu else n
        return [h.detach(), F.conv2d(n, conv2.weight.to(dt), conv2.bias.to(dt), padding=KS2 // 2).detach()]
    return conv1, gn, conv2, x, silu, ref(torch.float64), ref(torch.float32)


# ------------------------------------------------------------------------------------------------ attention
def attn_input(S, C, L, scale, key_shift, seed, tie=False):
    """qkv (S, 3C, L) = scale u, float32.  K gets a per-channel constant +-key_shift (moves every score of a row together:
    the softmax is unchanged, the running maximum is not).  Two keys of the LAST 128-key block (L-1, L-3) are made the
    largest key of query rows 5 and L/2; tie: keys 2 and 7 are identical and the maximum of row 9."""
    x = scale * _u((S, 3, C, L), seed)
    q, k = x[:, 0], x[:, 1]
    k[:, :, L - 1] = 0.8 * q[:, :, 5]
    k[:, :, L - 3] = 0.8 * q[:, :, L // 2]
    if tie:
        k[:, :, 2] = 0.8 * q[:, :, 9]
        k[:, :, 7] = k[:, :, 2]
    sign = torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0).double()
    k += key_shift * sign[None, :, None]
    return x.reshape(S, 3 * C, L).float()


def attn_forward_f64(qkv):
    """-> (out (S, C, L), P (S, L, L)) of softmax(Q^T K / sqrt(C)) applied to V, float64."""
    S, C3, L = qkv.shape
    C = C3 // 3
    q, k, v = qkv.double().reshape(S, 3, C, L).unbind(1)
    s = torch.bmm(q.transpose(1, 2), k) / math.sqrt(C)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    p = p / p.sum(-1, keepdim=True)
    return torch.bmm(v, p.transpose(1, 2)), p


def attn_ref(qkv, dy):
    """qkv (S, 3C, L), dy (S, C, L) -> (r64, r32): each [out, dqkv]; r64 closed form in float64, r32 stock fp32 torch."""
    S, C3, L = qkv.shape
    C = C3 // 3
    alpha = 1.0 / math.sqrt(C)
    q, k, v = qkv.double().reshape(S, 3, C, L).unbind(1)
    o, p = attn_forward_f64(qkv)
    dO = dy.double()
    dp = torch.bmm(dO.transpose(1, 2), v)                                  # [i][j]
    ds = p * (dp - (dO * o).sum(1)[:, :, None])
    dq = alpha * torch.bmm(k, ds.transpose(1, 2))
    dk = alpha * torch.bmm(q, ds)
    dv = torch.bmm(dO, p)
    r64 = [o, torch.stack([dq, dk, dv], 1).reshape(S, C3, L)]

    def f32(x):
        qq, kk, vv = x.reshape(S, 3, C, L).unbind(1)
        pp = torch.softmax(torch.bmm(qq.transpose(1, 2), kk) / math.sqrt(C), -1)
        return torch.bmm(vv, pp.transpose(1, 2))
    return r64, _grads(f32, (qkv,), dy)


def max_prob(qkv):
    return float(attn_forward_f64(qkv)[1].max(-1).values.mean())


# ------------------------------------------------------------------------------------------------ view softmax
def compose_views(N):
    """The two samples' view counts (B = 2): ragged where N allows."""
    return [N, max(1, N // 2)]


def compose_input(B, N, H, W, logit_scale, seed):
    """-> unet_out (S, 6, H, W) (noise channels O(1), view-weight logits logit_scale u), target, y_t, z (B, 3, H, W); float32."""
    assert B == 2
    S = sum(compose_views(N))
    out = torch.cat([1.5 * _u((S, 3, H, W), seed), logit_scale * _u((S, 3, H, W), seed + 1)], 1)
    return (out.float(), _u((B, 3, H, W), seed + 2).float(), _u((B, 3, H, W), seed + 3).float(),
            _u((B, 3, H, W), seed + 4).float())


def compose_fwd(out, vc, stock):
    """Reference view_fusion.py's composition: softmax over each sample's views of the logits, weighted sum of the noise
    channels -> (noise_hat (B, 3, H, W), weights (B, maxV, 3, H, W), zero past a sample's views).  stock: torch.softmax on
    the -inf padded stack (as the reference does it); otherwise restated with exp."""
    B, vmax = len(vc), max(vc)
    _, _, H, W = out.shape
    nh, ws, o = [], [], 0
    for b in range(B):
        eps, lg = out[o:o + vc[b], :3], out[o:o + vc[b], 3:]
        o += vc[b]
        if stock:
            w = torch.softmax(lg, 0)
        else:
            w = torch.exp(lg - lg.max(0, keepdim=True).values)
            w = w / w.sum(0, keepdim=True)
        nh.append((eps * w).sum(0))
        ws.append(torch.cat([w, w.new_zeros(vmax - vc[b], 3, H, W)]))
    return torch.stack(nh), torch.stack(ws)


def huber(d, delta=1.0):
    a = d.abs()
    return torch.where(a <= delta, 0.5 * d * d, delta * (a - 0.5 * delta))


def compose_ref(out, target, vc, penalty, gscale=1.7):
    """-> (r64, r32): each [noise_hat, weights, loss, d(gscale loss)/d out]; loss = mean rho(noise_hat - target),
    rho = "mse" d^2 | "huber" (delta 1)."""
    def run(o, t, stock):
        def f(x):
            nh, w = compose_fwd(x, vc, stock)
            d = nh - t
            if penalty == "mse":
                loss = F.mse_loss(nh, t) if stock else (d * d).mean()
            else:
                loss = F.huber_loss(nh, t, delta=1.0) if stock else huber(d).mean()
            f.keep = (nh.detach(), w.detach(), loss.detach())
            return loss * gscale
        x = o.clone().requires_grad_(True)
        f(x).backward()
        return [*f.keep, x.grad]
    return run(out.double(), target.double(), False), run(out, target, True)


def tail_ref(out, y_t, z, t, sched, vc):
    """The reverse step behind the composition (reference p_sample: y0_hat clamped, posterior mean, + z sigma) on the
    fp32 schedule tables -> (r64, r32): each [y_next, mean, weights]."""
    def run(dt, stock):
        nh, w = compose_fwd(out.to(dt), vc, stock)
        pick = lambda k: sched[k][t].to(dt).reshape(-1, 1, 1, 1)
        y0 = (pick("sqrt_recip_gammas") * y_t.to(dt) - pick("sqrt_recipm1_gammas") * nh).clamp(-1, 1)
        mean = pick("posterior_mean_coef1") * y0 + pick("posterior_mean_coef2") * y_t.to(dt)
        return [mean + z.to(dt) * (0.5 * pick("posterior_log_variance_clipped")).exp(), mean, w]
    return run(torch.float64, False), run(torch.float32, True)


# ------------------------------------------------------------------------------------------------ the GPU grid, by name
GN_SHAPES = [(64, 64, 64), (32, 16, 16), (192, 8, 8), (96, 8, 8), (64, 6, 10), (32, 5, 5)]      # (C, H, W)
GN_SILU = {(64, 64, 64): True, (32, 16, 16): False, (192, 8, 8): True, (96, 8, 8): False, (64, 6, 10): True, (32, 5, 5): False}
GN_CASES = [(r, s, None) for r in GN_RATIOS for s in GN_SIGMAS] + [(10, 1.0, "const"), (10, 1.0, "outlier")]
ATTN_SHAPES = [(64, 16, 16, 1), (32, 16, 16, 17), (192, 16, 16, 97), (64, 8, 8, 3), (96, 8, 8, 3), (32, 32, 32, 2)]      # (C, H, W, S)
STREAM_SHAPES = [(64, 10, 20, 2), (96, 10, 20, 2), (64, 16, 24, 2), (96, 16, 24, 2), (192, 10, 20, 2), (64, 7, 29, 2)]
ATTN_CASES = [(sc, sh, False) for sc in ATTN_SCALES for sh in ATTN_SHIFTS] + [(14, 8, True)]
COMPOSE_CASES = [(N, ls) for N in (1, 2, 23) for ls in COMPOSE_SCALES]
CONV_GN_SHAPES = [(6, 128, 64, 64, "vf_wino_conv_fwd_gn"), (1, 384, 192, 16, "vf_conv_fwd_gn")]      # (S, Cin, Cout, H, entry)
CONV_SMALL_SHAPES = [(64, 64, 64, 16, 3), (96, 320, 100, 8, 1)]                                      # (C0, C1, C2, H, KS2)
CONV_SMALL_RATIOS = [10, 100]
