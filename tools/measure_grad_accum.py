"""Measurements behind profiles/grad_accum.md (one process, one GPU, small UNet 64x64):

  1. the accumulate launch alone (and the plain Adam launch beside it) on the model's 33.9 M parameters: device events
     around 50 back-to-back launches, 5 rounds -> us per launch and TB/s over 12 (8 on the first micro-batch) / 28 B per
     parameter;
  2. the replayed step at B = 16, N = 6 with accum_steps = 1, 2, 4: three Trainers alternating, 6 rounds of 20 steps;
  3. what one set of weight packs costs (kind "pack" of an instrumented eager step);
  4. torch.cuda.max_memory_allocated over 4 steps of a fresh Trainer, eager and graph, accum_steps = 1, 2, 4.

    python tools/measure_grad_accum.py [--out result.json]
"""
import ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from view_fusion_amd import train, ops, _lib

dev = torch.device("cuda:0")
out = {}

def ev_time(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us

# 1. the launches alone on the small UNet's parameters
model = train.build_model(device="cuda:0", seed=0)
params = list(model.parameters())
numel = sum(p.numel() for p in params)
from view_fusion_amd.optim import FusedAdam
opt = FusedAdam(params, lr=1e-4)
grads = [torch.randn_like(p) * 1e-3 for p in params]
def setg():
    for p, g in zip(params, grads):
        p.grad = g
setg(); opt.accumulate(0.5, True); setg(); opt.accumulate(0.5, False); opt.step()
a = opt._acc_plan
raw = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
def acc_launch():
    _lib.call("vf_grad_accum_multi", ctypes.c_void_p(a["dev"][a["flip"]].data_ptr()), len(a["params"]), a["blocks"],
              ctypes.c_void_p(opt._acc_scal.data_ptr()), raw)
def set_beta(first):
    _lib.call("vf_adam_set_scalars", ctypes.c_void_p(opt._acc_scal.data_ptr()), 0.0 if first else 1.0, 0.5, 0.0, raw)
b = opt._plans[0]["buckets"][0]
def adam_launch():
    _lib.call("vf_adam_multi", ctypes.c_void_p(b["dev"][b["flip"]].data_ptr()), len(b["params"]), b["blocks"], 1e-4, 0.9, 0.999,
              1e-8, 0.5, 0.5, raw)
res = {}
for rnd in range(5):
    set_beta(False); acc_launch()
    res.setdefault("accum_us", []).append(ev_time(acc_launch, 50))
    set_beta(True); acc_launch()
    res.setdefault("accum_first_us", []).append(ev_time(acc_launch, 50))
    adam_launch()
    res.setdefault("adam_us", []).append(ev_time(adam_launch, 50))
med = lambda v: sorted(v)[len(v) // 2]
out["launch"] = dict(numel=numel, accum_us=res["accum_us"], accum_first_us=res["accum_first_us"], adam_us=res["adam_us"],
                     accum_TBs=12.0 * numel / med(res["accum_us"]) / 1e6, accum_first_TBs=8.0 * numel / med(res["accum_first_us"]) / 1e6,
                     adam_TBs=28.0 * numel / med(res["adam_us"]) / 1e6)
print(json.dumps(out["launch"]), flush=True)
del opt, grads, model, params
torch.cuda.empty_cache()

# 2. whole step at B = 16, N = 6, graph mode: A = 1, 2, 4 alternating
batch = train.synthetic_batch(16, 6, 64, dev, seed=0)
trs = {}
for A in (1, 2, 4):
    m = train.build_model(device="cuda:0", seed=0)
    trs[A] = train.Trainer(m, graph=True, accum_steps=A)
    for _ in range(4):
        trs[A].step(batch)
    torch.cuda.synchronize()
    print("A", A, "mode", trs[A].mode, "graph_steps", trs[A].graph_steps, "graphs", len(trs[A]._graphs), flush=True)
steps = {A: [] for A in trs}
for rnd in range(6):
    for A, tr in trs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            loss = tr.step(batch)
        torch.cuda.synchronize()
        steps[A].append((time.perf_counter() - t0) / 20 * 1e3)
out["step_ms"] = {A: dict(median=med(v), min=min(v), max=max(v)) for A, v in steps.items()}
out["graph_steps"] = {A: tr.graph_steps for A, tr in trs.items()}
print(json.dumps(out["step_ms"]), flush=True)

# 3. what one set of weight packs costs (an instrumented eager A = 1 step; kind "pack")
ops.st.KERNEL_LOG = []
trs[1].step(batch)
torch.cuda.synchronize()
log, ops.st.KERNEL_LOG = ops.st.KERNEL_LOG, None
pack = [r for r in log if r[0] == "pack"]
out["pack"] = dict(launches=len(pack), us=sum(r[2].elapsed_time(r[3]) for r in pack) * 1e3)
print(json.dumps(out["pack"]), flush=True)
del trs
torch.cuda.empty_cache()

# 4. peak memory, eager and graph, A = 1, 2, 4 (fresh trainer each; peak over 4 steps, relative to before the trainer)
out["peak"] = {}
for graph in (False, True):
    for A in (1, 2, 4):
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        m = train.build_model(device="cuda:0", seed=0)
        tr = train.Trainer(m, graph=graph, accum_steps=A)
        for _ in range(4):
            tr.step(batch)
        torch.cuda.synchronize()
        out["peak"][f"{'graph' if graph else 'eager'}_A{A}"] = dict(base_MiB=base / 2 ** 20, peak_MiB=torch.cuda.max_memory_allocated() / 2 ** 20,
                                                                   reserved_MiB=torch.cuda.max_memory_reserved() / 2 ** 20)
        del tr, m
print(json.dumps(out["peak"]), flush=True)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
