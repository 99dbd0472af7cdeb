"""Measurements behind profiles/level_sampler.md (one process, one GPU, BASELINE C2: small UNet 64x64, B = 16, N = 6,
S = 96 views, the replayed training step):

  the default step (uniform timesteps: the launches of the commit before the level sampler) against the step with
  model.set_level_sampler("loss_aware") and against a "fixed" proposal: three seeded Trainers alternating, 6 rounds of 20
  replayed steps each, host wall clock around synchronised rounds.

    python tools/measure_level_sampler.py [--out result.json] [--root <another checkout of this repository>]

--root imports view_fusion_amd from another checkout (built there): on one without set_level_sampler -- the parent commit --
only the default step is measured, which is how the default step is compared across commits (run both in turn on one
machine; profiles/guidance.md records a process-to-process spread of about 1 %).
"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
import torch
from view_fusion_amd import train

dev = torch.device("cuda:0")
med = lambda v: sorted(v)[len(v) // 2]
B, N, HW = 16, 6, 64
batch = train.synthetic_batch(B, N, HW, dev, seed=0)
cases = {"default": None}
if hasattr(train.ViewFusion, "set_level_sampler"):
    cases["loss_aware"] = dict(kind="loss_aware", warmup=1)                  # ready after the first steps: the table is in use
    cases["fixed"] = dict(kind="fixed", bins=64, probs=[1.0 + (k % 7) for k in range(64)])
trs = {}
for name, kw in cases.items():
    m = train.build_model(device="cuda:0", seed=0)
    if kw:
        m.set_level_sampler(**kw)
    trs[name] = train.Trainer(m, graph=True, seed=1)
    for _ in range(40 if name == "loss_aware" else 4):                       # (64 bins x warmup 1: every bin seen)
        trs[name].step(batch)
    torch.cuda.synchronize()
    print(name, "mode", trs[name].mode, "graph_steps", trs[name].graph_steps, flush=True)
steps = {k: [] for k in trs}
for rnd in range(6):
    for name, tr in trs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            loss = tr.step(batch)
        torch.cuda.synchronize()
        steps[name].append((time.perf_counter() - t0) / 20 * 1e3)
out = {"root": ROOT, "step_ms": {k: dict(median=med(v), min=min(v), max=max(v), rounds=v) for k, v in steps.items()},
       "graph_steps": {k: tr.graph_steps for k, tr in trs.items()}}
if "loss_aware" in trs:
    p, seen, ready = trs["loss_aware"].level_proposal()
    out["loss_aware_proposal"] = dict(ready=bool(ready), p_min=float(p.min()), p_max=float(p.max()),
                                      seen_min=int(seen.min()), seen_max=int(seen.max()))
print(json.dumps(out), flush=True)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
