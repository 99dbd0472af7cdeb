"""Measurements behind profiles/threshold.md (one process, one GPU, small UNet 64x64).

  python tools/measure_threshold.py sampler [--baseline]
      the replayed B = 1 reverse step at N = 1 / 6 / 12 with guidance=3.0 alone, with threshold=0.995, with
      guidance_rescale=0.7 and with both: wall time of a seeded K = 100 and a K = 20 chain (ddim, eta = 1: the tail draws
      its own z), ms/step = (K100 - K20) / 80 so that what a generate() call costs once (capture, warm-up step,
      snapshots, the scratch buffers) cancels; 5 rounds, the configurations alternating.
      --baseline: the default step (no guidance, no threshold) only -- the form that also runs on a tree from before the
      feature, for the yardstick "the default step is unchanged".
  python tools/measure_threshold.py kernels
      the three launches of the new tail alone, B = 1 and B = 16 at 64 x 64 and B = 1 at 128 x 192: HIP-event time of 200
      back-to-back calls of each entry point, and of ops.abs_quantile on the same sizes.
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import SMALL, SCHED_TEST  # noqa: E402
from view_fusion_amd import UNet, ViewFusion, ops  # noqa: E402
from view_fusion_amd.utils import deterministic_fill_  # noqa: E402

dev = torch.device("cuda:0")
med = lambda v: sorted(v)[len(v) // 2]


def model():
    net = UNet(**SMALL)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": SCHED_TEST}).eval()
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


def timed(vf, args, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = vf.generate(*args, seed=3, eta=1.0, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    return time.perf_counter() - t0


def sampler(baseline):
    vf = model()
    cases = {"none": {}} if baseline else {
        "g3": dict(guidance=3.0), "g3+threshold": dict(guidance=3.0, threshold=0.995),
        "g3+rescale": dict(guidance=3.0, guidance_rescale=0.7),
        "g3+both": dict(guidance=3.0, threshold=0.995, guidance_rescale=0.7)}
    res = {}
    for N in (1, 6, 12):
        g = torch.Generator().manual_seed(1)
        args = (torch.rand(1, N, 3, 64, 64, generator=g).to(dev), torch.tensor([N]), torch.rand(1, 1, generator=g).to(dev))
        for kw in cases.values():
            timed(vf, args, sample_steps=2, **kw)             # warm: weight packing, allocator
        per = {k: [] for k in cases}
        for rnd in range(5):
            for name, kw in cases.items():
                w100, w20 = timed(vf, args, sample_steps=100, **kw), timed(vf, args, sample_steps=20, **kw)
                per[name].append(1e3 * (w100 - w20) / 80)
        res[f"N{N}"] = {k: dict(median=round(med(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in per.items()}
        print(f"N={N} ms/step " + "  ".join(f"{k}: median {med(v):.4f} ({min(v):.4f} ... {max(v):.4f})" for k, v in per.items()),
              flush=True)
    print(json.dumps({"sampler_ms_per_step": res, "baseline": baseline}), flush=True)


def _event_us(fn, reps=200):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def kernels():
    vf = model()
    res = {}
    for B, N, H, W in ((1, 6, 64, 64), (16, 6, 64, 64), (1, 2, 128, 192)):
        g = torch.Generator().manual_seed(2)
        S = B * N
        out = torch.randn(S + B, 6, H, W, generator=g).to(dev)
        y = torch.randn(B, 3, H, W, generator=g).to(dev)
        off, _, max_v = ops.view_offsets([N] * B, dev)
        t = torch.full((B,), 500, device=dev)
        gs = ops.guidance_scales(dev, B, 3.0)
        scratch = ops.threshold_scratch(y)
        kw = dict(seed=3, guidance=gs, S=S, inplace=False, want_weights=True)
        row = {
            "tail_cfg_rng": _event_us(lambda: ops.p_sample_tail(out, off, y, None, t, vf._sched(), B, max_v, True, **kw)),
            "three_launches": _event_us(lambda: ops.p_sample_tail(out, off, y, None, t, vf._sched(), B, max_v, True,
                                                                 threshold=0.995, guidance_rescale=0.7, scratch=scratch, **kw)),
            "rescale_only": _event_us(lambda: ops.p_sample_tail(out, off, y, None, t, vf._sched(), B, max_v, True,
                                                               guidance_rescale=0.7, scratch=scratch, **kw)),
            "abs_quantile": _event_us(lambda: ops.abs_quantile(y.reshape(B, -1), 0.995)),
        }
        res[f"B{B}_N{N}_{H}x{W}"] = {k: round(v, 2) for k, v in row.items()}
        print(f"B={B} N={N} {H}x{W} us per call (back to back, launch overhead included): {res[f'B{B}_N{N}_{H}x{W}']}", flush=True)
    print(json.dumps({"kernel_us": res}), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "sampler":
        sampler("--baseline" in sys.argv)
    else:
        kernels()
