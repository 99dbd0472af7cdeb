#!/usr/bin/env python3
"""SHA-256 digests of everything the loss kernels and the stacking kernels write, over a grid of every path they have:
the bit-for-bit gate of a change that must not alter them (the companion of tools/tail_bits.py for the training step).

    python tools/loss_bits.py --out new.json                                # on the commit under test
    python tools/loss_bits.py --out old.json --root ../parent               # the package of another checkout (its parent)
    python tools/loss_bits.py --compare old.json new.json                   # no GPU: exit status 1 on any difference

It calls only ops.compose_loss, ops.compose_mse_loss and ops.stack_views (and the schedule's tables), with inputs from
a seeded CPU generator (no UNet), so the same file runs on any commit that has those.  One process, a few seconds.

Shapes (those of tests/test_gpu_loss_options.py, for its reasons): 8 x 8 with views (1, 3, 2) -- fewer float4s than one
workgroup; 12 x 20 with (1, 3, 2) -- n4 % 256 != 0; 128 x 192 with views (2,) -- more than 64 * 256 float4s per sample:
the grid-stride loop and all 64 partials.
Grid: prediction {eps, v, x0} x penalty {mse, l1, huber with delta = 0.7} x weighting {None, min_snr(5), p2(1, 1),
trunc_snr} x sample_scale {None, given} x softmax / mean x hist {None, 5 bins holding earlier sums and counts};
compose_mse_loss, softmax / mean, is the control that must not move.
Digests: loss, sample_loss, the weight (want_weight=True), unet_out.grad of (1.7 loss).backward(), bin_sum, bin_cnt.
The hybrid loss (vlb=, keys NAME/vlb/...): the same three shapes on a NINE-channel output, prediction x penalty x softmax /
mean x hist x lambda {0.001, 0}, under min_snr(5); t in 1..T-1 and c1, hi, lo of a 20-step linear schedule
(schedule.variance_tables); the digests above and sample_vlb.
Stacking (ops.stack_views, keys NAME/stack/...): 8 x 8 and 12 x 20 with views (1, 3, 2), Cc {3, 6} x drop {None, given} x
null_rows x self_cond {None, zeros by sc_channels=True, given} x noise {None, given} x copy_cond into an x that holds
0.25 everywhere; digests of x, level_s, angle_s.  (No drop, no null rows and no self_cond is the plain kernel: a control.)
"""
import argparse
import hashlib
import itertools
import json
import os
import sys

SHAPES = {"8x8": ((8, 8), (1, 3, 2)), "12x20": ((12, 20), (1, 3, 2)), "128x192": ((128, 192), (2,))}
LEVELS = {3: [0.95, 0.4, 0.05], 1: [0.95]}
PREDICTIONS = ("eps", "v", "x0")
PENALTIES = ("mse", "l1", "huber")
WEIGHTS = ((None, 0.0, 0.0), ("min_snr", 5.0, 0.0), ("p2", 1.0, 1.0), ("trunc_snr", 0.0, 0.0))
DELTA, BINS, GLOSS = 0.7, 5, 1.7
VLB_T, VLB_STEPS, VLB_LAMBDAS = 20, {3: [1, 7, 19], 1: [7]}, (0.001, 0.0)
STACK_SHAPES = ("8x8", "12x20")


def digest(t):
    if t is None:
        return None
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def loss_cases(torch, ops, dev, name, out):
    (H, W), vc = SHAPES[name]
    B, S = len(vc), sum(vc)
    g = torch.Generator().manual_seed(1000 * H + W)
    unet = (2.0 * torch.randn(S, 6, H, W, generator=g)).to(dev)
    noise, y_0 = torch.randn(B, 3, H, W, generator=g).to(dev), (2.0 * torch.rand(B, 3, H, W, generator=g) - 1.0).to(dev)
    level = torch.tensor(LEVELS[B], device=dev)
    scale = (0.25 + 2.0 * torch.rand(B, generator=g)).to(dev)
    off, _, _ = ops.view_offsets(list(vc), dev)
    for weighting in (1, 0):
        og = unet.clone().requires_grad_(True)
        loss = ops.compose_mse_loss(og, noise, off, B, weighting)
        (loss * GLOSS).backward()
        out[f"{name}/compose_mse_loss/w{weighting}"] = dict(loss=digest(loss), grad=digest(og.grad))
    for pred, pen, (kind, a, b), scaled, weighting, hist in itertools.product(PREDICTIONS, PENALTIES, WEIGHTS, (0, 1),
                                                                              (1, 0), (0, 1)):
        og = unet.clone().requires_grad_(True)
        bins = None
        if hist:
            bins = (torch.full((BINS,), 0.5, device=dev), torch.full((BINS,), 3, dtype=torch.int32, device=dev))
        kw = dict(y_0=y_0) if pred != "eps" else {}
        loss, sl, w = ops.compose_loss(og, noise, off, B, weighting, level, pen, DELTA, kind, a, b, hist=bins,
                                       sample_scale=scale if scaled else None, want_weight=True, prediction=pred, **kw)
        (loss * GLOSS).backward()
        out[f"{name}/{pred}/{pen}/{kind}/scale{scaled}/w{weighting}/hist{hist}"] = dict(
            loss=digest(loss), sample_loss=digest(sl), weight=digest(w), grad=digest(og.grad),
            bin_sum=digest(bins[0]) if hist else None, bin_cnt=digest(bins[1]) if hist else None)


def vlb_cases(torch, ops, schedule, dev, name, out):
    (H, W), vc = SHAPES[name]
    B, S = len(vc), sum(vc)
    g = torch.Generator().manual_seed(2000 * H + W)
    unet = (2.0 * torch.randn(S, 9, H, W, generator=g)).to(dev)
    noise, y_0 = torch.randn(B, 3, H, W, generator=g).to(dev), (2.0 * torch.rand(B, 3, H, W, generator=g) - 1.0).to(dev)
    level = torch.tensor(LEVELS[B], device=dev)
    betas = schedule.make_beta_schedule("linear", VLB_T, 1e-4, 0.09)
    c1 = schedule.schedule_tensors(betas, dev)["posterior_mean_coef1"]
    hi, lo = (torch.tensor(v, dtype=torch.float32, device=dev) for v in schedule.variance_tables(betas))
    t = torch.tensor(VLB_STEPS[B], dtype=torch.int64, device=dev)
    off, _, _ = ops.view_offsets(list(vc), dev)
    for pred, pen, lam, weighting, hist in itertools.product(PREDICTIONS, PENALTIES, VLB_LAMBDAS, (1, 0), (0, 1)):
        og = unet.clone().requires_grad_(True)
        bins = None
        if hist:
            bins = (torch.full((BINS,), 0.5, device=dev), torch.full((BINS,), 3, dtype=torch.int32, device=dev))
        kw = dict(y_0=y_0) if pred != "eps" else {}
        loss, sl, w, sv = ops.compose_loss(og, noise, off, B, weighting, level, pen, DELTA, "min_snr", 5.0, 0.0, hist=bins,
                                           want_weight=True, prediction=pred, vlb=(t, c1, hi, lo, lam), **kw)
        (loss * GLOSS).backward()
        out[f"{name}/vlb/{pred}/{pen}/lam{lam}/w{weighting}/hist{hist}"] = dict(
            loss=digest(loss), sample_loss=digest(sl), weight=digest(w), sample_vlb=digest(sv), grad=digest(og.grad),
            bin_sum=digest(bins[0]) if hist else None, bin_cnt=digest(bins[1]) if hist else None)


def stack_cases(torch, ops, dev, name, out):
    (H, W), vc = SHAPES[name]
    B, S = len(vc), sum(vc)
    g = torch.Generator().manual_seed(3000 * H + W)
    y_t, noise, sc = (torch.randn(B, 3, H, W, generator=g).to(dev) for _ in range(3))
    level, angle = torch.tensor(LEVELS[B], device=dev), torch.rand(B, 1, generator=g).to(dev)
    drop = torch.tensor([1, 0, 1][:B], dtype=torch.uint8, device=dev)
    off, _, _ = ops.view_offsets(list(vc), dev)
    for Cc in (3, 6):
        y_cond = torch.randn(B, max(vc), Cc, H, W, generator=g).to(dev)
        for dropped, null_rows, sc_mode, noisy, copy_cond in itertools.product((0, 1), (0, 1), ("none", "zeros", "given"),
                                                                               (0, 1), (1, 0)):
            x = torch.full((S + B if null_rows else S, Cc + (3 if sc_mode == "none" else 6), H, W), 0.25, device=dev)
            kw = {} if sc_mode == "none" else dict(self_cond=sc if sc_mode == "given" else None, sc_channels=True)
            x, ls, as_ = ops.stack_views(y_cond, y_t, noise if noisy else None, level, angle, off, S, x=x,
                                         copy_cond=bool(copy_cond), drop=drop if dropped else None,
                                         null_rows=bool(null_rows), **kw)
            out[f"{name}/stack/cc{Cc}/drop{dropped}/null{null_rows}/sc_{sc_mode}/noise{noisy}/copy{copy_cond}"] = dict(
                x=digest(x), level_s=digest(ls), angle_s=digest(as_))


def compare(new, old):
    """Two {case: {name: digest}} -> the sorted cases that are missing on one side or differ in any digest."""
    return sorted(k for k in set(new) | set(old) if new.get(k) != old.get(k))


def report(new, old, label):
    bad = compare(new, old)
    for k in bad[:40]:
        print("DIFFERENT:", k, {n: "=" if (new.get(k) or {}).get(n) == (old.get(k) or {}).get(n) else "!="
                                for n in (new.get(k) or old.get(k))})
    print(f"{len(bad)} of {len(set(new) | set(old))} cases differ from {label}")
    return 1 if bad else 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="where the JSON of digests goes (runs the grid on cuda:0)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose view_fusion_amd is imported (default: this file's)")
    ap.add_argument("--compare", nargs="+", metavar="JSON", help="with --out: one JSON of another run to compare the new "
                    "digests with; alone: two JSONs to compare (no GPU).  Exit status 1 unless every digest is equal")
    args = ap.parse_args(argv)
    if args.out is None:
        if not args.compare or len(args.compare) != 2:
            ap.error("without --out, --compare takes the two files to compare")
        old, new = (json.load(open(p))["digests"] for p in args.compare)
        return report(new, old, args.compare[0])
    import torch
    sys.path.insert(0, os.path.abspath(args.root))
    from view_fusion_amd import ops, schedule
    dev = torch.device("cuda:0")
    digests = {}
    for name in SHAPES:
        loss_cases(torch, ops, dev, name, digests)
        vlb_cases(torch, ops, schedule, dev, name, digests)
    for name in STACK_SHAPES:
        stack_cases(torch, ops, dev, name, digests)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(cases=len(digests), root=os.path.abspath(args.root), digests=digests), f, indent=0, sort_keys=True)
    print(f"{len(digests)} cases, {sum(v is not None for d in digests.values() for v in d.values())} digests -> {args.out}")
    if args.compare:
        return report(digests, json.load(open(args.compare[0]))["digests"], args.compare[0])
    return 0


if __name__ == "__main__":
    sys.exit(main())
