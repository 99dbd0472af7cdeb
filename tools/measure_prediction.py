"""Measurements behind profiles/prediction.md (tools/measure_loss_options.py's method: one GPU, small UNet 64x64, B = 16,
N = 6: S = 96 views; a Trainer in graph mode, rounds of 20 replayed steps timed on the host around a device sync).

One process measures ONE tree and ONE prediction, so that the step under "v" can be set against the default step of the
commit before the feature: run this file once per process, alternating between the two checkouts, and compare the
medians; two processes of the same tree give the process-to-process spread.

    python tools/measure_prediction.py --prediction v   [--root <checkout>] [--out result.json]
    python tools/measure_prediction.py --prediction eps  --root <checkout of the parent commit>

--root: the checkout to import view_fusion_amd from (default: this file's).  With "eps" nothing of the feature is called,
so the same file measures a checkout that does not have it.  Also prints the launches of one eager step's loss
(forward + backward) and the loss pair alone on a (96, 6, 64, 64) output.
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--prediction", default="eps", choices=("eps", "v", "x0"))
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
from view_fusion_amd import ops, train  # noqa: E402

dev = torch.device("cuda:0")
med = lambda v: sorted(v)[len(v) // 2]
B, N, HW = 16, 6, 64
out = dict(root=os.path.abspath(args.root), prediction=args.prediction)


def ev_time(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us


# 1. the loss pair alone (min_snr, so that "eps" runs the loss-option kernels the prediction kernels are siblings of)
g = torch.Generator().manual_seed(0)
unet_out = torch.randn(B * N, 6, HW, HW, generator=g).to(dev).requires_grad_(True)
noise, y_0 = (torch.randn(B, 3, HW, HW, generator=g).to(dev) for _ in range(2))
level = (0.05 + 0.9 * torch.rand(B, generator=g)).to(dev)
off, S, _ = ops.view_offsets([N] * B, dev)
pred_kw = {} if args.prediction == "eps" else dict(prediction=args.prediction, y_0=y_0)


def pair():
    loss, _ = ops.compose_loss(unet_out, noise, off, B, True, level, "mse", 1.0, "min_snr", 5.0, 0.0, **pred_kw)
    torch.autograd.grad(loss, unet_out)


pair()
out["loss_pair_us"] = [ev_time(pair, 200) for _ in range(5)]
out["loss_pair_us_median"] = med(out["loss_pair_us"])
print(json.dumps({k: out[k] for k in ("prediction", "loss_pair_us_median", "loss_pair_us")}), flush=True)

# 2. the replayed training step, default objective
batch = train.synthetic_batch(B, N, HW, dev, seed=0)
m = train.build_model(device="cuda:0", seed=0)
if args.prediction != "eps":
    m.set_prediction(args.prediction)
ops.st.KERNEL_LOG = []
try:
    m(y_cond=batch["y_cond"], view_count=batch["view_count"], angle=batch["angle"], y_0=batch["y_0"]).backward()
    names = [r[5] for r in ops.st.KERNEL_LOG]
finally:
    ops.st.KERNEL_LOG = None
m.zero_grad(set_to_none=True)
out["eager_step_launches"] = len(names)
out["loss_launches"] = [n for n in names if n.startswith("vf_compose")]
tr = train.Trainer(m, graph=True)
for _ in range(4):
    tr.step(batch)
torch.cuda.synchronize()
out["mode"], out["graph_steps"] = tr.mode, tr.graph_steps
steps = []
for rnd in range(args.rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        loss = tr.step(batch)
    torch.cuda.synchronize()
    steps.append((time.perf_counter() - t0) / 20 * 1e3)
out["step_ms"] = dict(median=med(steps), min=min(steps), max=max(steps), rounds=steps)
out["loss"] = float(loss)
print(json.dumps({k: out[k] for k in ("prediction", "eager_step_launches", "loss_launches", "mode", "graph_steps", "step_ms",
                                      "loss")}), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
