"""Measurements behind profiles/loss_options.md (one process, one GPU, small UNet 64x64, B = 16, N = 6: S = 96 views):

  1. the loss launches alone on a (96, 6, 64, 64) output: the MSE pair (vf_compose_fwd with a target + vf_compose_mse_bwd)
     against the loss-option pair (vf_compose_loss_fwd + vf_compose_loss_bwd: huber, min_snr, 10 bins): device events
     around 200 back-to-back forward + backward pairs, 5 rounds, alternating;
  2. the replayed training step: the default objective (the launches of the commit before the loss options) against
     min_snr + loss_bins=10 and against huber + p2 + loss_bins=10: three Trainers alternating, 6 rounds of 20 steps.

    python tools/measure_loss_options.py [--out result.json]
"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from view_fusion_amd import train, ops

dev = torch.device("cuda:0")
out = {}
med = lambda v: sorted(v)[len(v) // 2]


def ev_time(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us


# 1. the launches alone
B, N, HW = 16, 6, 64
g = torch.Generator().manual_seed(0)
unet_out = torch.randn(B * N, 6, HW, HW, generator=g).to(dev).requires_grad_(True)
target = torch.randn(B, 3, HW, HW, generator=g).to(dev)
level = torch.rand(B, generator=g).to(dev)
off, S, _ = ops.view_offsets([N] * B, dev)
hist = (torch.zeros(10, device=dev), torch.zeros(10, device=dev, dtype=torch.int32))


def mse_pair():
    loss = ops.compose_mse_loss(unet_out, target, off, B, True)
    torch.autograd.grad(loss, unet_out)


def opt_pair():
    loss, _ = ops.compose_loss(unet_out, target, off, B, True, level, "huber", 1.0, "min_snr", 5.0, 0.0, hist=hist)
    torch.autograd.grad(loss, unet_out)


res = {"mse_pair_us": [], "option_pair_us": []}
mse_pair(); opt_pair()
for rnd in range(5):
    res["mse_pair_us"].append(ev_time(mse_pair, 200))
    res["option_pair_us"].append(ev_time(opt_pair, 200))
out["launches"] = dict(res, mse_median=med(res["mse_pair_us"]), option_median=med(res["option_pair_us"]),
                       note="host-enqueued pairs: three launches each, allocation and autograd included")
print(json.dumps(out["launches"]), flush=True)

# 2. the replayed step
batch = train.synthetic_batch(B, N, HW, dev, seed=0)
cases = {"default": (None, None), "min_snr+bins10": (dict(weighting="min_snr"), 10),
         "huber+p2+bins10": (dict(penalty="huber", weighting="p2"), 10)}
trs = {}
for name, (loss_kw, bins) in cases.items():
    m = train.build_model(device="cuda:0", seed=0)
    if loss_kw:
        m.set_loss(**loss_kw)
    trs[name] = train.Trainer(m, graph=True, loss_bins=bins)
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
            loss = tr.step(batch)
        torch.cuda.synchronize()
        steps[name].append((time.perf_counter() - t0) / 20 * 1e3)
out["step_ms"] = {k: dict(median=med(v), min=min(v), max=max(v), rounds=v) for k, v in steps.items()}
out["graph_steps"] = {k: tr.graph_steps for k, tr in trs.items()}
mean, count = trs["min_snr+bins10"].loss_by_level()
out["loss_by_level"] = dict(mean=[None if x != x else x for x in mean.tolist()], count=count.tolist())
print(json.dumps(out["step_ms"]), flush=True)
print(json.dumps(out["loss_by_level"]), flush=True)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
