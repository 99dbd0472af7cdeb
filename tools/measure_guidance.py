"""Measurements behind profiles/guidance.md (one process, one GPU, small UNet 64x64).

  python tools/measure_guidance.py sampler [--baseline]
      the replayed B = 1 reverse step at N = 1 / 6 / 12 with guidance=None and guidance=3.0: wall time of a seeded
      K = 100 and a K = 20 chain (ddim, eta = 1: the tail draws its own z), ms/step = (K100 - K20) / 80 so that what a
      generate() call costs once (capture, warm-up step, snapshots) cancels; 5 rounds, the configurations alternating.
      --baseline: guidance=None only -- the form that also runs on a tree from before the feature, for the yardstick
      "the default step is unchanged".
  python tools/measure_guidance.py train
      one replayed C2 training step (B = 16, N = 6) with set_cond_dropout(0.1) against the default: two seeded Trainers
      alternating, 6 rounds of 20 steps.
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
from view_fusion_amd import UNet, ViewFusion, train  # noqa: E402
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
    cases = {"none": {}} if baseline else {"none": {}, "g3": dict(guidance=3.0)}
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


def training():
    B, N, HW = 16, 6, 64
    batch = train.synthetic_batch(B, N, HW, dev, seed=0)
    trs = {}
    for name, p in (("default", 0.0), ("cond_dropout_0.1", 0.1)):
        m = train.build_model(device="cuda:0", seed=0)
        m.set_cond_dropout(p)
        trs[name] = train.Trainer(m, graph=True, seed=0)
        for _ in range(4):
            trs[name].step(batch)
        torch.cuda.synchronize()
        print(name, "mode", trs[name].mode, "graph_steps", trs[name].graph_steps, flush=True)
    steps = {k: [] for k in trs}
    for rnd in range(6):
        for name, tr in trs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                tr.step(batch)
            torch.cuda.synchronize()
            steps[name].append((time.perf_counter() - t0) / 20 * 1e3)
    print(json.dumps({"train_step_ms": {k: dict(median=round(med(v), 4), min=round(min(v), 4), max=round(max(v), 4))
                                        for k, v in steps.items()}}), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "sampler":
        sampler("--baseline" in sys.argv)
    else:
        training()
