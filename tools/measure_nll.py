"""Measurements behind profiles/nll.md (tools/measure_learned_variance.py's method: one GPU, small UNet 64x64, B = 16, N = 6:
S = 96 views; timed on the host around a device sync).

One process measures ONE tree and ONE mode: run this file once per process, alternating between the modes, and compare
the medians; two processes of the same mode give the process-to-process spread.

    python tools/measure_nll.py --mode forward [--lv]     # one eager no-grad forward at S rows: level gather, stacking, UNet
    python tools/measure_nll.py --mode bound [--lv]       # one step of ViewFusion.bound_terms: the same plus three launches
    python tools/measure_nll.py --mode kernels [--lv]     # the three launches alone (noisy target, term, finish), per step

"bound" times bound_terms at two chain lengths (K = 10 and K = 50): the difference is 40 steps, free of the per-call
part (tables, buffers, the prior).  --lv: the nine-channel network with a learned variance.
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="bound", choices=("forward", "bound", "kernels"))
ap.add_argument("--lv", action="store_true", help="the 9-channel model with a learned variance")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
from view_fusion_amd import ops, schedule, train  # noqa: E402

dev = torch.device("cuda:0")
med = lambda v: sorted(v)[len(v) // 2]          # noqa: E731
B, N, HW = 16, 6, 64
NINE = dict(train.SMALL_UNET, out_channel=9)
out = dict(root=os.path.abspath(args.root), mode=args.mode, lv=args.lv)

m = train.build_model(NINE if args.lv else None, device="cuda:0", phase="test", seed=0)
if args.lv:
    m.set_learned_variance()
m.eval()
batch = train.synthetic_batch(B, N, HW, dev, seed=0)
y_0 = batch["y_0"] * 2 - 1
T = m.num_timesteps


def host_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3   # ms


if args.mode == "forward":
    off, S, _ = ops.view_offsets(batch["view_count"], dev)
    t = torch.full((B,), T // 2, device=dev, dtype=torch.long)
    with torch.no_grad():
        x, _ = m._denoise(y_0, batch["y_cond"], batch["angle"], t, off, S)

        def fwd():
            for _ in range(40):
                m._denoise(y_0, batch["y_cond"], batch["angle"], t, off, S, x=x, copy_cond=False)

        fwd()
        per = [host_time(fwd) / 40 for _ in range(args.rounds)]
    out["forward_ms"] = dict(median=med(per), min=min(per), max=max(per), S=S)
elif args.mode == "bound":
    run = lambda k: m.bound_terms(batch["y_cond"], batch["view_count"], batch["angle"], y_0, seed=1, sample_steps=k)  # noqa: E731
    run(10)
    per = []
    for _ in range(args.rounds):
        t10, t50 = host_time(lambda: run(10)), host_time(lambda: run(50))
        per.append((t50 - t10) / 40)
    out["bound_step_ms"] = dict(median=med(per), min=min(per), max=max(per))
    out["bpd"] = float(run(10)["total_bpd"].mean())
else:
    off, S, _ = ops.view_offsets(batch["view_count"], dev)
    tau = schedule.sample_timesteps(T, 50)
    tab = {k: torch.tensor(v, dtype=torch.float32, device=dev)
           for k, v in schedule.nll_tables(m.betas64, tau, m.prediction).items()}
    tau_d = torch.tensor(tau, dtype=torch.int64, device=dev)
    kidx = torch.full((B,), 25, device=dev, dtype=torch.int64)
    ids = ops.sample_ids(dev, B)
    unet_out = torch.randn(S, 9 if args.lv else 6, HW, HW, device=dev)
    y_k = torch.empty_like(y_0)
    res = (torch.zeros(B, 50, device=dev), torch.zeros(B, 50, device=dev))
    scratch = ops.nll_scratch(B, dev)

    def three():
        for _ in range(200):
            ops.nll_noisy(y_0, kidx, tau_d, m.gammas, seed=1, ids=ids, out=y_k)
            ops.nll_terms(unet_out, off, y_k, y_0, kidx, tab, B, True, learned=args.lv, out=res, scratch=scratch)

    three()
    per = [host_time(three) / 200 * 1e3 for _ in range(args.rounds)]
    out["three_launches_us"] = dict(median=med(per), min=min(per), max=max(per))

print(json.dumps(out), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
