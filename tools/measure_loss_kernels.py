"""us per forward + backward pair of every loss path alone (profiles/loss_templates.md), tools/measure_tail_kernels.py's
method: (96, 6, 64, 64) output (B = 16, N = 6), softmax weighting; the MSE pair (the control), eps / v / x0 with min_snr,
eps with huber + p2 + 10 bins, eps and v with a sample_scale, and the hybrid loss of a learned variance (lv/...: a
(96, 9, 64, 64) output, vlb= with lambda = 0.001 on a 1000-step linear schedule) for eps and v.  Each path is captured as a graph of 50 pairs and replayed 10
times per round, 7 rounds: device time per pair (three launches) without the host.  Uses only ops.compose_loss and
ops.compose_mse_loss, so it runs on any commit that has them; run it from the root of the tree to be measured:
python tools/measure_loss_kernels.py"""
import json, os, sys
import torch
sys.path.insert(0, os.getcwd())
from view_fusion_amd import ops, schedule
dev = torch.device("cuda:0")
med = lambda v: sorted(v)[len(v) // 2]
B, N, H, W = 16, 6, 64, 64
g = torch.Generator().manual_seed(5)
unet = torch.randn(B * N, 6, H, W, generator=g).to(dev).requires_grad_(True)
noise, y_0 = torch.randn(B, 3, H, W, generator=g).to(dev), torch.randn(B, 3, H, W, generator=g).to(dev)
level = (0.05 + 0.9 * torch.rand(B, generator=g)).to(dev)
scale = (0.5 + torch.rand(B, generator=g)).to(dev)
off, _, _ = ops.view_offsets([N] * B, dev)
bins = (torch.zeros(10, device=dev), torch.zeros(10, device=dev, dtype=torch.int32))
loss_of = lambda *a, **kw: ops.compose_loss(unet, noise, off, B, True, level, *a, **kw)[0]
unet9 = torch.randn(B * N, 9, H, W, generator=g).to(dev).requires_grad_(True)
betas = schedule.make_beta_schedule("linear", 1000, 1e-6, 1e-2)
hi, lo = (torch.tensor(v, dtype=torch.float32, device=dev) for v in schedule.variance_tables(betas))
vlb = (torch.randint(1, 1000, (B,), generator=g).to(dev), schedule.schedule_tensors(betas, dev)["posterior_mean_coef1"], hi, lo, 0.001)
lv_of = lambda *a, **kw: ops.compose_loss(unet9, noise, off, B, True, level, *a, vlb=vlb, **kw)[0]
paths = {"mse_pair": lambda: ops.compose_mse_loss(unet, noise, off, B, True),
         "eps/mse/min_snr": lambda: loss_of("mse", 1.0, "min_snr", 5.0, 0.0),
         "eps/huber/p2/bins": lambda: loss_of("huber", 1.0, "p2", 1.0, 1.0, hist=bins),
         "eps/mse/min_snr/scale": lambda: loss_of("mse", 1.0, "min_snr", 5.0, 0.0, sample_scale=scale),
         "v/mse/min_snr": lambda: loss_of("mse", 1.0, "min_snr", 5.0, 0.0, prediction="v", y_0=y_0),
         "v/l1/min_snr/scale": lambda: loss_of("l1", 1.0, "min_snr", 5.0, 0.0, sample_scale=scale, prediction="v", y_0=y_0),
         "x0/mse/min_snr": lambda: loss_of("mse", 1.0, "min_snr", 5.0, 0.0, prediction="x0", y_0=y_0),
         "lv/eps/mse/min_snr": lambda: lv_of("mse", 1.0, "min_snr", 5.0, 0.0),
         "lv/v/huber/min_snr/bins": lambda: lv_of("huber", 1.0, "min_snr", 5.0, 0.0, hist=bins, prediction="v", y_0=y_0)}
res = {}
for name, fn in paths.items():
    pair = lambda: torch.autograd.grad(fn(), unet9 if name.startswith("lv/") else unet)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(5):
            pair()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(50):
            pair()
    gr.replay(); torch.cuda.synchronize()
    us = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            gr.replay()
        e1.record(); torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / 500)
    res[name] = dict(median=round(med(us), 3), min=round(min(us), 3), max=round(max(us), 3))
    print(name, res[name], flush=True)
print(json.dumps({"loss_pair_us": res}), flush=True)
