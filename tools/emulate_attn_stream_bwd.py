"""CPU emulation of the streaming attention backward's recomputed probabilities (csrc/attention_stream.hip), fp32, the
score accumulated two channels per step as v_mfma_f32_32x32x2_f32 does:

    A  one fp32 log-sum-exp per query, -lse / alpha as the initial accumulator of the score product (the old kernel)
    B  (c2 max, 1 / sum) per query, the score accumulated from 0, p = exp2(c2 s - c2 max) / sum (the kernel now)

on the L = 200 streaming cases of tests/cond_ref.py at scale 14; prints d(qkv)'s err against float64, e and the bound.
    python tools/emulate_attn_stream_bwd.py"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import cond_ref as cr  # noqa: E402


def seq(q, k, acc0):
    acc = acc0.clone().float()
    for c in range(0, q.shape[1], 2):
        t = q[:, c, :, None].double() * k[:, c, None, :].double() + q[:, c + 1, :, None].double() * k[:, c + 1, None, :].double()
        acc = (acc.double() + t).float()
    return acc


def run(C, L, scale, shift, tie, S=2):
    qkv = cr.attn_input(S, C, L, scale, shift, 11, tie)
    dy = cr._u((S, C, L), 18).float()
    r64, r32 = cr.attn_ref(qkv, dy)
    alpha = torch.tensor(1.0 / math.sqrt(C), dtype=torch.float32)
    c2 = alpha * torch.tensor(1.44269504088896341, dtype=torch.float32)
    q, k, v = qkv.reshape(S, 3, C, L).unbind(1)
    s = seq(q, k, torch.zeros(S, L, L))                    # the forward's raw scores [i][j]
    m = s.max(-1, keepdim=True).values
    pf = torch.exp2(s * c2 - m * c2)
    l = pf.sum(-1, keepdim=True)
    o = torch.bmm(v, (pf / l).transpose(1, 2))
    dp = torch.bmm(dy.transpose(1, 2), v) - (dy * o).sum(1)[:, :, None]
    res = {}
    for name in "AB":
        if name == "A":
            s0 = -(alpha * m + torch.log(l)) / alpha
            p = torch.exp2(seq(q, k, s0.expand(S, L, L)) * c2)
        else:
            p = torch.exp2(s * c2 - m * c2) * (1.0 / l)
        ds = p * dp
        g = torch.stack([alpha * torch.bmm(k, ds.transpose(1, 2)), alpha * torch.bmm(q, ds), torch.bmm(dy, p)], 1)
        res[name] = cr.err(g.reshape(S, 3 * C, L), r64[1])
    e = cr.err(r32[1], r64[1])
    print(f"({C}, L={L}) scale {scale} shift {shift}{' tie' if tie else ''}: e {e:.3e}  bound {cr.bound(e, cr.TOL['attn_bwd']):.3e}  "
          f"one lse {res['A']:.3e}  (max, 1/sum) {res['B']:.3e}")


if __name__ == "__main__":
    for C in (64, 96):
        for sc, sh, tie in cr.ATTN_CASES:
            if sc == 14:
                run(C, 200, sc, sh, tie)
