#!/usr/bin/env python3
"""SHA-256 digests of everything the reverse-step tails and stack_views write, over a grid of every path they have:
the bit-for-bit gate of a change that must not alter them.

    python tools/tail_bits.py --out new.json                      # on the commit under test
    python tools/tail_bits.py --out old.json                      # on its parent (a separate worktree)
    python tools/tail_bits.py --out new.json --compare old.json   # exit status 1 on any difference

It calls only ops.stack_views, ops.p_sample_tail, ops.sampler_step and ops.threshold_scratch, with inputs from a seeded
CPU generator (no UNet), so the same file runs on any commit that has those four.  One process, a few seconds.

Shapes: B = 3, view counts (1, 3, 2), Cout = 6, H x W = 8 x 8 (one partial workgroup), 20 x 20 (two chunks, the channel
boundaries inside a workgroup) and 152 x 152 (3 HW / 4 = 17 328 float4 > 64 * 256: a second trip of the grid-stride loop).
Tails: {ancestral, few-step} x eps {composed; guided, g = (0, 1, 3); eps buffer + threshold; eps buffer, guided,
threshold + rescale} x z {loaded, None, seed= with ids (7, 2^33 + 1, 0)} x softmax weighting on / off x want_weights
on / off; the ancestral tail with t = (0, 4, 9) and clip on / off (on only, under a threshold); the few-step tail with
kidx = (0, 1, 2) -- sigma = 0, c1 = 0, both non-zero --, with and without y0_prev, in place and not.
stack_views: {plain, drop, null_rows, both} x Cc {3, 6} x noise given / None x copy_cond 0 / 1.
Digests: y_next, mean, the weights, y0_prev after the call; x, level_s, angle_s.
"""
import argparse
import hashlib
import itertools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from view_fusion_amd import ops  # noqa: E402

VIEWS = (1, 3, 2)
SHAPES = ((8, 8), (20, 20), (152, 152))
T, K = 10, 4


def digest(t):
    if t is None:
        return None
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def tail_cases(dev, H, W, out):
    B, S, maxV = len(VIEWS), sum(VIEWS), max(VIEWS)
    g = torch.Generator().manual_seed(1000 * H + W)
    rand = lambda *s: torch.rand(*s, generator=g)
    randn = lambda *s: torch.randn(*s, generator=g)
    unet = (2.0 * randn(S + B, 6, H, W)).to(dev)             # rows S.. are the null rows of the guided cases
    y, z, hist = randn(B, 3, H, W).to(dev), randn(B, 3, H, W).to(dev), (0.8 * randn(B, 3, H, W)).to(dev)
    off = torch.tensor([0, 1, 4, 6], dtype=torch.int32, device=dev)
    ids = torch.tensor([7, 2 ** 33 + 1, 0], dtype=torch.int64, device=dev)
    scale = torch.tensor([0.0, 1.0, 3.0], device=dev)
    sched = {n: (lo + (hi - lo) * rand(T)).to(dev) for n, lo, hi in (
        ("sqrt_recip_gammas", 1.0, 1.6), ("sqrt_recipm1_gammas", 0.1, 1.2), ("posterior_log_variance_clipped", -6.0, -1.0),
        ("posterior_mean_coef1", 0.1, 0.9), ("posterior_mean_coef2", 0.1, 0.9))}
    tables = {n: (lo + (hi - lo) * rand(K)).to(dev) for n, lo, hi in (
        ("a", 1.0, 1.6), ("b", 0.1, 1.2), ("cy", 0.2, 0.9), ("c0", 0.2, 0.9), ("c1", -0.5, -0.1), ("sigma", 0.1, 0.6))}
    tables["sigma"][0] = 0.0
    tables["c1"][1] = 0.0
    tables["tau"] = torch.tensor([9, 6, 3, 0], dtype=torch.int64, device=dev)
    t = torch.tensor([0, 4, 9], dtype=torch.int64, device=dev)
    kidx = torch.tensor([0, 1, 2], dtype=torch.int64, device=dev)
    scratch = ops.threshold_scratch(y)
    sources = {"composed": {}, "guided": dict(guidance=scale, S=S),
               "threshold": dict(threshold=0.9, scratch=scratch),
               "guided+threshold+rescale": dict(guidance=scale, S=S, threshold=0.9, guidance_rescale=0.7,
                                                scratch=scratch)}
    noises = {"z": dict(z=z), "none": dict(z=None), "seed": dict(z=None, seed=1234567, ids=ids)}
    for (sn, src), (nn, noise), weighting, want in itertools.product(sources.items(), noises.items(), (1, 0), (1, 0)):
        uo = unet if "guidance" in src else unet[:S].contiguous()
        name = f"{H}x{W}/{sn}/{nn}/w{weighting}/ww{want}"
        for clip in ((True,) if "threshold" in src else (True, False)):
            y_next, mean, wts = ops.p_sample_tail(uo, off, y, noise["z"], t, sched, B, maxV, weighting, clip=clip,
                                                  want_weights=bool(want), want_mean=True,
                                                  **{k: v for k, v in noise.items() if k != "z"}, **src)
            out[f"ancestral/{name}/clip{int(clip)}"] = dict(y_next=digest(y_next), mean=digest(mean), weights=digest(wts))
        for with_hist, inplace in itertools.product((1, 0), (1, 0)):
            yy = y.clone()
            prev = hist.clone() if with_hist else None
            y_next, wts = ops.sampler_step(uo, off, yy, noise["z"], kidx, tables, B, maxV, weighting, y0_prev=prev,
                                           want_weights=bool(want), inplace=bool(inplace),
                                           **{k: v for k, v in noise.items() if k != "z"}, **src)
            out[f"few-step/{name}/hist{with_hist}/inplace{inplace}"] = dict(y_next=digest(y_next), weights=digest(wts),
                                                                             y0_prev=digest(prev))


def stack_cases(dev, H, W, out):
    B, S, Nmax = len(VIEWS), sum(VIEWS), max(VIEWS)
    g = torch.Generator().manual_seed(77 * H + W)
    off = torch.tensor([0, 1, 4, 6], dtype=torch.int32, device=dev)
    drop = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev)
    for Cc in (3, 6):
        y_cond = torch.rand(B, Nmax, Cc, H, W, generator=g).to(dev)
        y_t, noise = torch.randn(B, 3, H, W, generator=g).to(dev), torch.randn(B, 3, H, W, generator=g).to(dev)
        level, angle = torch.rand(B, generator=g).to(dev), torch.rand(B, 1, generator=g).to(dev)
        for use_drop, null_rows, with_noise, copy_cond in itertools.product((0, 1), (0, 1), (1, 0), (1, 0)):
            rows = S + B if null_rows else S
            x = torch.full((rows, Cc + 3, H, W), 0.25, device=dev)      # copy_cond = 0 leaves the conditioning half
            kw = {}
            if use_drop:
                kw["drop"] = drop
            if null_rows:
                kw["null_rows"] = True
            x, ls, as_ = ops.stack_views(y_cond, y_t, noise if with_noise else None, level, angle, off, S, x=x,
                                         copy_cond=bool(copy_cond), **kw)
            out[f"stack_views/{H}x{W}/Cc{Cc}/drop{use_drop}/null{null_rows}/noise{with_noise}/copy{copy_cond}"] = dict(
                x=digest(x), level_s=digest(ls), angle_s=digest(as_))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True, help="where the JSON of digests goes")
    ap.add_argument("--compare", help="a JSON written by another run: exit status 1 unless every digest is equal")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    digests = {}
    with torch.no_grad():
        for H, W in SHAPES:
            tail_cases(dev, H, W, digests)
            stack_cases(dev, H, W, digests)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(cases=len(digests), digests=digests), f, indent=0, sort_keys=True)
    print(f"{len(digests)} cases, {sum(v is not None for d in digests.values() for v in d.values())} digests -> {args.out}")
    if args.compare:
        other = json.load(open(args.compare))["digests"]
        bad = sorted(k for k in set(digests) | set(other) if digests.get(k) != other.get(k))
        for k in bad[:40]:
            print("DIFFERENT:", k, {n: "=" if (digests.get(k) or {}).get(n) == (other.get(k) or {}).get(n) else "!="
                                    for n in (digests.get(k) or other.get(k))})
        print(f"{len(bad)} of {len(set(digests) | set(other))} cases differ from {args.compare}")
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
