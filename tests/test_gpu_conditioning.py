"""The softmax / normalisation kernels on a real MI355X on HARD inputs (tests/cond_ref.py): group mean up to 100 standard
deviations at three scales, a constant group, an outlier pixel; attention logits to +-350 with a per-channel key shift, a
tie at the row maximum and the largest key in the last key block; view-weight logits to +-100.

One rule for all of them (cond_ref.judge): err = max|a - r64| / max|r64| against a float64 restatement, e = the same for
stock fp32 torch on the CPU on the same inputs, pass if err <= max(4 e, tol) with tol the family's stated tolerance
(cond_ref.TOL: tests/test_gpu_kernels.py); any non-finite value fails; e <= 2.5e-4 for every case (asserted, and
checked for the whole grid on the CPU in tests/test_cond_host.py, which also shows that a one-pass variance, a softmax
without its maximum and a stale block maximum FAIL this rule on these inputs).  Every case confirms its route through
ops.st.KERNEL_LOG and the library's own shape predicates; none may skip.  Measured values: profiles/conditioning.md."""
import ctypes

import pytest
import torch

import cond_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _judge_all(label, names, got, r64, r32, tols, extra=0.0):
    """Print every figure, then assert the rule for every output."""
    extras = extra if isinstance(extra, tuple) else (extra,) * len(names)
    rows = [(n, *cr.judge(a, b, c, t, x)) for n, a, b, c, t, x in zip(names, got, r64, r32, tols, extras)]
    print()                                                       # (pytest -s: off the test's progress line)
    for n, d, e, b, ok in rows:
        print(f"COND | {label} | {n} | e {e:.3e} | err {d:.3e} | bound {b:.3e} | {'ok' if ok else 'FAIL'}")
    assert all(r[4] for r in rows), [(r[0], r[1], r[3]) for r in rows if not r[4]]


class _Log:
    """with _Log() as names: ... -> the C-ABI entry points launched inside, in order."""

    def __enter__(self):
        from view_fusion_amd import ops
        ops.st.KERNEL_LOG = []
        self.names = []
        return self.names

    def __exit__(self, *exc):
        from view_fusion_amd import ops
        torch.cuda.synchronize()
        self.names.extend(e[5] for e in ops.st.KERNEL_LOG)
        ops.st.KERNEL_LOG = None


# ------------------------------------------------------------------------------------------------ GroupNorm
def _gn_case(C, H, W, ratio, sigma, variant):
    x = cr.gn_input(2, C, H, W, ratio, sigma, 21, variant)
    ga, be, dy = cr.gn_params(2, C, H, W, 21)
    return (x, ga, be, dy, *cr.gn_ref(x, ga, be, dy, cr.GN_SILU[(C, H, W)]))


@pytest.mark.parametrize("ratio,sigma,variant", cr.GN_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("C,H,W", cr.GN_SHAPES)
def test_group_norm_conditioning(dev, C, H, W, ratio, sigma, variant):
    """csrc/norm.hip's register kernels (two-pass statistics; (192, 8x8): the 16-lane segment backward) and
    csrc/norm_any.hip (maps that are no power of two), forward and every gradient.  Constant group: the forward of that
    group is held to the DERIVED bound 2 ulp32(c) |gamma|max / sqrt(eps) around act(beta) (a mean one ulp off is
    legitimate), the other groups to the common rule and the gradients to it with that term added to the floor."""
    from view_fusion_amd import ops
    x, ga, be, dy, r64, r32 = _gn_case(C, H, W, ratio, sigma, variant)
    silu, HW = cr.GN_SILU[(C, H, W)], H * W
    pow2 = HW & (HW - 1) == 0
    # route: the single-pass register backward exactly on the power-of-two maps, the general kernels on the others
    assert bool(ops._lib.load().vf_gn_bwd_emits_rowsum(C, HW, 32)) == pow2
    xg, gg, bg = (t.to(dev).requires_grad_(True) for t in (x, ga, be))
    with _Log() as names:
        y = ops.group_norm(xg, gg, bg, 32, silu)
        y.backward(dy.to(dev))
    assert [n for n in names if "colsum" not in n] == ["vf_gn_fwd", "vf_gn_cat_bwd"], names
    got = [y, xg.grad, gg.grad, bg.grad]
    extra = 0.0
    if variant == "const":
        cpg, term = C // 32, cr.const_group_term(ga)
        want = cr.act(be[cpg:2 * cpg], silu)[:, None, None].expand(cpg, H, W)
        dev_c = float((y.detach()[0, cpg:2 * cpg].double().cpu() - want).abs().max())
        print(f"\nCOND | gn ({C},{H}x{W}) const group | max abs(y - act(beta)) {dev_c:.3e} | derived bound {2 * term:.3e}")
        assert bool(torch.isfinite(y).all()) and dev_c <= 2 * term
        mask = torch.ones(2, C, 1, 1, dtype=torch.bool)
        mask[0, cpg:2 * cpg] = False                              # the common rule on every other group
        got[0], r64, r32 = y.cpu() * mask, [r64[0] * mask, *r64[1:]], [r32[0] * mask, *r32[1:]]
        extra = (0.0, term, term, term)                           # (the forward's other groups: the plain rule)
    _judge_all(f"gn ({C},{H}x{W}) ratio {ratio} sigma {sigma:g} {variant or ''}", ("y", "dx", "dgamma", "dbeta"), got, r64, r32,
               (cr.TOL["gn_fwd"],) + (cr.TOL["gn_bwd"],) * 3, extra)


@pytest.mark.parametrize("ratio", cr.GN_RATIOS)
@pytest.mark.parametrize("S,Cin,Cout,H,entry", cr.CONV_GN_SHAPES)
def test_conv_fused_group_norm_conditioning(dev, S, Cin, Cout, H, entry, ratio):
    """The GroupNorm evaluated behind a conv without autograd (ops.conv2d_gn): the Winograd fix-up launch
    (csrc/winograd24.hip) and the split-K reduce launch of the direct conv (csrc/conv.hip), under the natural policy."""
    from view_fusion_amd import ops
    conv, gn, x, vb, res, r64, r32 = cr.conv_gn_case(S, Cin, Cout, H, ratio)
    conv, gn = conv.to(dev), gn.to(dev)
    with torch.no_grad(), _Log() as names:
        y, a = ops.conv2d_gn(x.to(dev), conv, gn, 32, True, view_bias=vb.to(dev), residual=res.to(dev), want_y=True)
    assert [n for n in names if "pack" not in n] == [entry], names
    _judge_all(f"{entry} ({Cin}->{Cout},{H}x{H},S={S}) ratio {ratio}", ("y", "gn(y)"), (y, a), r64, r32,
               (cr.TOL["conv_gn"],) * 2)


@pytest.mark.parametrize("ratio", cr.CONV_SMALL_RATIOS)
@pytest.mark.parametrize("C0,C1,C2,H,KS2", cr.CONV_SMALL_SHAPES)
def test_conv_small_statistics_conditioning(dev, C0, C1, C2, H, KS2, ratio):
    """conv -> GroupNorm(32)[+Swish] -> conv with the GroupNorm folded into the second conv's staging from the first
    conv's integer sums (vf_conv_small_gn, driven as test_conv_small_groupnorm_without_a_launch does), with the first
    conv's bias putting the group mean at `ratio` standard deviations.  The variance is E[x^2] - mean^2 of those sums: it
    has to be formed in double from sums that are exact to the fixed-point unit (in fp32 it loses ~6e-4 at ratio 100)."""
    from view_fusion_amd import _lib
    S = 2
    conv1, gn, conv2, x, silu, r64, r32 = cr.conv_small_case(C0, C1, C2, H, KS2, ratio, S)
    hg = r64[0].reshape(S, 32, -1)
    assert float((hg.mean(-1).abs() / hg.std(-1)).max()) > 0.85 * ratio         # the case is what it says
    conv1, conv2, gn = conv1.to(dev), conv2.to(dev), gn.to(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st_raw = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(xin, conv, in_stats, out_stats):
        Cout, Cin, KS, _ = conv.weight.shape
        y = torch.empty(S, Cout, H, H, device=dev)
        wp = None
        if KS == 3 and Cin % 32 == 0:
            wp = torch.empty(_lib.load().vf_conv_small_pack_floats(Cout, Cin), device=dev)
            _lib.call("vf_conv_small_pack", P(conv.weight.detach()), P(wp), Cout, Cin, st_raw)
        _lib.call("vf_conv_small_gn", P(xin), None, 0, P(conv.weight.detach()), P(conv.bias.detach()), None, None, P(y), S,
                  Cin, Cout, H, H, KS, P(in_stats), P(gn.weight.detach()) if in_stats is not None else None,
                  P(gn.bias.detach()) if in_stats is not None else None, 32 if in_stats is not None else 0, 1e-5, int(silu),
                  P(out_stats), None, None, 0, 0, None, None, P(wp), 0, st_raw)
        return y

    outs = []
    for _ in range(2):
        st = torch.zeros(S * C1 * 2, dtype=torch.int64, device=dev)
        h = launch(x.to(dev), conv1, None, st)
        y = launch(h, conv2, st, None)
        outs.append((h.clone(), st.clone(), y.clone()))
    torch.cuda.synchronize()
    (h, st, y), (h2, st2, y2) = outs
    assert torch.equal(st, st2) and torch.equal(y, y2)                # integer atomics: bit-reproducible
    # the sums of the h the kernel wrote, to the fixed-point unit: one rounding to 2^-24 (half a unit) per 16-pixel tile,
    # plus what this check's own float64 sum of H H terms can be off by (H H 2^-53 of the sum of magnitudes)
    sums = st.view(S, C1, 2).double().cpu() / 2.0 ** 24
    hd, tiles = h.double().cpu(), H * H // 16
    for k, t in enumerate((hd, hd * hd)):
        own = float(t.abs().sum((2, 3)).max()) * H * H * 2.0 ** -53
        d = float((sums[..., k] - t.sum((2, 3))).abs().max())
        print(f"\nCOND | vf_conv_small_gn integer sum {k} | off by {d:.3e} | derived bound {tiles * 2.0 ** -25 + own:.3e}")
        assert d <= tiles * 2.0 ** -25 + own
    _judge_all(f"vf_conv_small_gn ({C0}->{C1}->{C2},{H}x{H},{KS2}x{KS2}) ratio {ratio}", ("h", "y"), (h, y), r64, r32,
               (cr.TOL["small_h"], cr.TOL["small_y"]))


# ------------------------------------------------------------------------------------------------ attention
def _attn_case(C, H, W, S, scale, shift, tie):
    qkv = cr.attn_input(S, C, H * W, scale, shift, 11, tie)
    dy = cr._u((S, C, H * W), 18).float()
    return (qkv, dy, *cr.attn_ref(qkv, dy))


ATTN_KERNEL = {(64, 16, 16, 1): "q16", (32, 16, 16, 17): "q32", (192, 16, 16, 97): "128-query", (64, 8, 8, 3): "q16",
               (96, 8, 8, 3): "split", (32, 32, 32, 2): "generic"}
ATTN_KERNEL_CODE = {1: "q16", 2: "q32", 3: "split", 4: "128-query"}       # vf_attention_fwd_kernel (include/vf_hip.h)


def _attn_launches(C, L):
    """The C-ABI entries of a training call of ops.attention (forward, then backward)."""
    if L == 256 and C % 32 == 0:
        return ["vf_attention_fwd", "vf_attention_dscore"] + (["vf_attention_dvdk"] if C % 64 == 0 else ["vf_bgemm"] * 2)
    if L == 64 and C % 32 == 0:          # (C % 32 != 0 sends the fused maps to the generic path too)
        return ["vf_attention_fwd", "vf_bgemm", "vf_softmax_bwd", "vf_bgemm", "vf_bgemm", "vf_bgemm"]
    return ["vf_bgemm", "vf_softmax_fwd", "vf_bgemm", "vf_bgemm", "vf_softmax_bwd", "vf_bgemm", "vf_bgemm", "vf_bgemm"]


@pytest.mark.parametrize("scale,shift,tie", cr.ATTN_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("C,H,W,S", cr.ATTN_SHAPES)
def test_attention_conditioning(dev, C, H, W, S, scale, shift, tie):
    """ops.attention forward and d(qkv): the 16-query kernel (L = 256 and L = 64), the 32-query kernel in both roles
    (forward; dS + dQ), the 128-query kernel (S = 97: the smallest S the launcher's cost rule sends there), the L = 64
    key-split kernel (C = 96: no multiple of 64) with the five-launch backward, the generic materialised-score path."""
    from view_fusion_amd import ops
    qkv, dy, r64, r32 = _attn_case(C, H, W, S, scale, shift, tie)
    # the route: ops' choice of path, and inside vf_attention_fwd the kernel the launcher itself says it takes here
    kernel, launches = ATTN_KERNEL[(C, H, W, S)], _attn_launches(C, H * W)
    assert ops.attention_route(C, H * W) == ("generic" if kernel == "generic" else "fused")
    if kernel != "generic":
        assert ATTN_KERNEL_CODE[ops._lib.load().vf_attention_fwd_kernel(S, C, H * W)] == kernel
    qg = qkv.reshape(S, 3 * C, H, W).to(dev).requires_grad_(True)
    with _Log() as names:
        o = ops.attention(qg)
        o.backward(dy.reshape(S, C, H, W).to(dev))
    assert names == launches, names
    _judge_all(f"attention {kernel} ({C},{H}x{W},S={S}) scale {scale} shift {shift}{' tie' if tie else ''}", ("out", "dqkv"),
               (o.reshape(S, C, -1), qg.grad.reshape(S, 3 * C, -1)), r64, r32, (cr.TOL["attn_fwd"], cr.TOL["attn_bwd"]))


@pytest.mark.parametrize("scale,shift,tie", cr.ATTN_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("C,H,W,S", cr.STREAM_SHAPES)
def test_attention_streaming_conditioning(dev, C, H, W, S, scale, shift, tie):
    """ops.attention_streaming (csrc/attention_stream.hip: online softmax over 128-key blocks; the backward recomputes
    the probabilities from the forward's saved (scaled maximum, 1 / sum)): L = 200 (ragged second block) and L = 384
    (three blocks, two rescales); rows 5 and L/2 meet their largest key in the last block.  (Recomputed from ONE fp32
    log-sum-exp, d(qkv) missed the rule at L = 200, scale 14: profiles/conditioning.md.)"""
    from view_fusion_amd import ops
    qkv, dy, r64, r32 = _attn_case(C, H, W, S, scale, shift, tie)
    qg = qkv.reshape(S, 3 * C, H, W).to(dev).requires_grad_(True)
    with _Log() as names:
        o = ops.attention_streaming(qg)
        o.backward(dy.reshape(S, C, H, W).to(dev))
    assert names == ["vf_attn_stream_fwd", "vf_attn_stream_bwd"], names
    _judge_all(f"attention stream ({C},L={H * W},S={S}) scale {scale} shift {shift}{' tie' if tie else ''}", ("out", "dqkv"),
               (o.reshape(S, C, -1), qg.grad.reshape(S, 3 * C, -1)), r64, r32, (cr.TOL["attn_fwd"], cr.TOL["attn_bwd"]))


# ------------------------------------------------------------------------------------------------ view softmax
@pytest.mark.parametrize("N,logit_scale", cr.COMPOSE_CASES)
def test_view_softmax_conditioning(dev, N, logit_scale):
    """vf_compose_fwd (weights + noise_hat), vf_compose_mse_bwd, vf_compose_loss_fwd / _bwd with the Huber penalty, and the
    composition inside vf_p_sample_tail, at one view, two and 23 (ragged: the second sample has N // 2), 16x16."""
    from oracle import view_fusion_ref as vfr
    from view_fusion_amd import ops
    B, H = 2, 16
    out, target, y_t, z = cr.compose_input(B, N, H, H, logit_scale, 31)
    vc = cr.compose_views(N)
    off, S, maxv = ops.view_offsets(vc, dev)
    assert (S, maxv) == (sum(vc), N)
    tol = (cr.TOL["compose"], cr.TOL["compose"], cr.TOL["compose_loss"], cr.TOL["compose"])     # noise_hat, weights, loss, dout
    label = f"compose N {N} logits {logit_scale}"

    r64, r32 = cr.compose_ref(out, target, vc, "mse")
    og = out.to(dev).requires_grad_(True)
    with _Log() as names:
        nh, w = ops.compose(out.to(dev), off, B, maxv, True)
        loss = ops.compose_mse_loss(og, target.to(dev), off, B, True)
        (loss * 1.7).backward()
    assert names == ["vf_compose_fwd", "vf_compose_fwd", "vf_compose_mse_bwd"], names
    _judge_all(label + " mse", ("noise_hat", "weights", "loss", "dout"), (nh, w, loss, og.grad), r64, r32, tol)

    r64, r32 = cr.compose_ref(out, target, vc, "huber")
    og = out.to(dev).requires_grad_(True)
    with _Log() as names:
        loss, _ = ops.compose_loss(og, target.to(dev), off, B, True, torch.full((B,), 0.5, device=dev), penalty="huber")
        (loss * 1.7).backward()
    assert names == ["vf_compose_loss_fwd", "vf_compose_loss_bwd"], names
    _judge_all(label + " huber", ("loss", "dout"), (loss, og.grad), r64[2:], r32[2:], tol[2:])

    sched = vfr.schedule_buffers(vfr.beta_schedule("linear", 1000, 1e-4, 0.09))
    t = torch.tensor([400, 1])
    r64, r32 = cr.tail_ref(out, y_t, z, t, sched, vc)
    with _Log() as names:
        y, m, w2 = ops.p_sample_tail(out.to(dev), off, y_t.to(dev), z.to(dev), t.to(dev), {k: v.to(dev) for k, v in sched.items()},
                                     B, maxv, True, want_mean=True)
    assert names == ["vf_p_sample_tail"], names
    _judge_all(label + " tail", ("y_next", "mean", "weights"), (y, m, w2), r64, r32, (cr.TOL["compose"],) * 3)
