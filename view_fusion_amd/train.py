"""Synthetic-data training / sampling harness for the ViewFusion hot path.

Mirrors the reference's iteration semantics (experiment.py:90-120 model/optimizer/DDP setup,
:265-293 the step: set LR -> zero_grad -> model(...) -> backward -> Adam.step) without its
dataset, wandb and checkpoint plumbing.  One process per GPU; gradients are averaged over RCCL
(backend "nccl" on ROCm) by the gradient arena of reducer.py -- the backward kernels write into the
communication buffer, one all-reduce per segment overlaps the rest of the backward pass -- or, with
VF_REDUCER=ddp, by torch's DistributedDataParallel as in the reference.
"""
import contextlib
import math
import os

import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel

from . import reducer
from .unet import UNet
from .view_fusion import ViewFusion

SMALL_UNET = dict(in_channel=6, out_channel=6, inner_channel=64, norm_groups=32, channel_mults=(1, 2, 3, 5),
                  attn_res=(16,), res_blocks=3, image_size=64)          # configs/small-v100.yaml:19-30
BETA_SCHEDULE = {
    "train": dict(schedule="linear", num_timesteps=2000, linear_start=1e-6, linear_end=1e-2),
    "test": dict(schedule="linear", num_timesteps=1000, linear_start=1e-4, linear_end=0.09),
}                                                                        # configs/small-v100.yaml:9-18


class LrScheduler:
    """Linear warm-up to `peak_lr` over `peak_it`, then peak * decay_rate**(dt/decay_it)
    (reference utils/schedulers.py, constants from experiment.py:112-117)."""

    def __init__(self, peak_lr=1e-4, peak_it=2500, decay_rate=0.16, decay_it=4000000):
        self.peak_lr, self.peak_it, self.decay_rate, self.decay_it = peak_lr, peak_it, decay_rate, decay_it

    def get_cur_lr(self, it):
        if it < self.peak_it:
            return self.peak_lr * (it / self.peak_it)
        return self.peak_lr * self.decay_rate ** ((it - self.peak_it) / self.decay_it)


def init_rccl_group(local_rank, rank=None, world_size=None):
    """RCCL ("nccl" on ROCm) process group for one rank per GPU.  RCCL's kernels run on HIGH-PRIORITY streams: the
    compute kernels of this engine (one 512-thread Winograd workgroup per CU, all of its LDS and registers) leave no
    room for a collective's workgroups to co-reside, so the segment all-reduces that the gradient arena issues during
    the backward pass can only run when a CU frees up between workgroup rounds -- with priority they get those CUs
    first instead of queueing behind the whole next conv launch.  Knobs left to the environment (RCCL defaults are
    kept): NCCL_ALGO / NCCL_PROTO / NCCL_MIN_NCHANNELS; the payload is 6 segments of ~22 MiB per step, so the
    bandwidth-optimal ring / direct algorithms apply, not the latency ones."""
    torch.cuda.set_device(local_rank)
    kw = {} if rank is None else dict(rank=rank, world_size=world_size)
    try:
        opts = dist.ProcessGroupNCCL.Options(is_high_priority_stream=True)
        dist.init_process_group(backend="nccl", pg_options=opts, device_id=torch.device("cuda", local_rank), **kw)
    except (AttributeError, TypeError):          # a torch build without the option object
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank), **kw)


def init_distributed():
    """(rank, local_rank, world).  torchrun env -> process group; else single process.

    Backend: RCCL ("nccl" on ROCm) over xGMI, one rank per GPU, as the reference (utils/dist.py:21).  Two knobs exist
    for exercising the multi-rank code path on a box with fewer GPUs than ranks (tests/test_gpu_bench_two_rank.py):
    VF_DIST_BACKEND=gloo selects the gloo transport (RCCL refuses two ranks on one device) and VF_SHARE_GPU=1 maps
    rank r to device r % device_count.  The process group is created BEFORE the first HIP call of the process."""
    if "WORLD_SIZE" not in os.environ or int(os.environ["WORLD_SIZE"]) <= 1:
        return 0, 0, 1
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    backend = os.environ.get("VF_DIST_BACKEND", "nccl" if torch.cuda.device_count() > 0 else "gloo")
    if os.environ.get("VF_SHARE_GPU") == "1" and torch.cuda.device_count() > 0:
        local_rank %= torch.cuda.device_count()
    if backend == "nccl":
        init_rccl_group(local_rank)
    else:
        dist.init_process_group(backend=backend)
        if torch.cuda.device_count() > 0:
            torch.cuda.set_device(local_rank)
    return dist.get_rank(), local_rank, dist.get_world_size()


def synthetic_batch(B, N, hw, device, seed=0, ragged=False):
    """NMR-shaped random batch (data/nmr_dataset.py:10-52): images in [0,1], angle = 2pi/24*k."""
    g = torch.Generator().manual_seed(seed)
    y_0 = torch.rand(B, 3, hw, hw, generator=g)
    y_cond = torch.rand(B, N, 3, hw, hw, generator=g)
    angle = 2 * math.pi / 24 * torch.randint(0, 24, (B, 1), generator=g).float()
    view_count = torch.randint(1, N + 1, (B,), generator=g) if ragged else torch.full((B,), N)
    return dict(y_0=y_0.to(device), y_cond=y_cond.to(device), angle=angle.to(device), view_count=view_count)


def build_model(unet_params=None, beta_schedule=None, device="cuda", phase="train", weighting=True, seed=0):
    torch.manual_seed(seed)
    net = UNet(**(unet_params or SMALL_UNET))
    vf = ViewFusion(net, beta_schedule or BETA_SCHEDULE, weighting, weighting).to(device)
    vf.set_new_noise_schedule(device=torch.device(device), phase=phase)
    return vf


def step_sample_ids(it, B, rank=0, world=1, global_batch=None):
    """First sample id of this rank's batch at iteration `it` of a seeded run; sample b of the batch has id + b.
    id = it * global_batch + rank * B + b with global_batch = world * B by default: the ids of an iteration are the
    same set however the global batch is split over ranks, and no id repeats across iterations."""
    if global_batch is None:
        global_batch = world * B
    if (rank + 1) * B > global_batch:
        raise ValueError(f"rank {rank} with a batch of {B} does not fit a global batch of {global_batch}")
    return it * global_batch + rank * B


def split_batch(batch, extra, accum_steps):
    """The per-step batch as `accum_steps` contiguous micro-batches along the batch dimension -> [(batch_m, extra_m)].
    Every per-sample input is cut -- tensors (views, no copies) and lists whose leading length is the batch size B:
    y_0, y_cond, angle, view_count (list, CPU or device tensor) and injected t / u / noise / sample_ids -- and anything
    else (the seed, None) is handed to every micro-batch as it is.  Micro-batch m holds samples m B/A ... (m+1) B/A - 1,
    so with the ids of step_sample_ids() it draws exactly what those samples draw in the undivided batch."""
    A, B = int(accum_steps), batch["y_0"].shape[0]
    if A < 1 or B % A:
        raise ValueError(f"accum_steps={accum_steps} does not divide the batch of {B} samples")
    n = B // A

    def cut(v, m):
        if torch.is_tensor(v):
            return v[m * n:(m + 1) * n] if v.dim() >= 1 and v.shape[0] == B else v
        if isinstance(v, (list, tuple)) and len(v) == B:
            return v[m * n:(m + 1) * n]
        return v

    return [({k: cut(v, m) for k, v in batch.items()}, {k: cut(v, m) for k, v in extra.items()}) for m in range(A)]


DISTILL_INPUTS = ("distill_z", "distill_level", "distill_eps", "distill_x0")     # ViewFusion.distill_targets


class _StepGraph:
    """One captured training iteration (forward, backward, Adam) for one batch geometry -- or, with accum_steps > 1, one
    captured micro-batch (forward, backward, the accumulate launch)."""
    __slots__ = ("graph", "inputs", "view_count", "off", "vc", "loss", "adam", "keep", "seen", "grads", "accum", "sample", "drop",
                 "level", "vlb")

    def __init__(self):
        self.graph, self.seen, self.accum = None, 0, None


class Trainer:
    """The reference's iteration (experiment.py:265-293) around `model`.

    graph (default: on; the VF_STEP_GRAPH=0 environment variable or graph=False turn it off): GPU runs replay the WHOLE
    iteration -- weight packs, forward, backward, the multi-tensor Adam launch: ~1000 kernels -- as one HIP graph per
    batch geometry instead of enqueueing it launch by launch.  The geometry is the tensor shapes plus the stacked-view
    count S = sum(view_count): which sample owns which views is the offsets table the kernels read from device memory,
    so it is a graph INPUT like the images, and a ragged run (experiment.py:277-279 draws view_count per sample and
    iteration) needs one graph per S it meets (at most B*(N-1)+1), not one per view_count vector.  A geometry is
    captured after it has run eagerly `GRAPH_AFTER` times (descriptor tables, packed-weight buffers and optimizer
    state then exist and are only re-used); up to `GRAPH_MAX` graphs share one memory pool (each keeps its own
    gradient tensors, 136 MB for the small UNet).  Eager as before: injected arguments other than the draws t / u /
    noise and the seeded draws' sample_ids (which are graph inputs; their seed is part of the geometry key), a device-resident view_count (reading it back would be a sync per step), a
    kernel log, torch DDP as the reducer (VF_REDUCER=ddp).  world > 1 with the gradient arena has three launch modes
    (`self.mode`): "split" (the default: forward + backward replayed, the six segment all-reduces and the Adam launch
    issued eagerly after each replay), "captured" (VF_CAPTURE_COLLECTIVES=1: the collectives recorded into the graph on
    RCCL's stream, Adam included; the default only for a group of one) and "eager".  A rank whose capture fails raises
    the arena's failure flag, which rides the gradient all-reduce; at iteration numbers all ranks compute alike
    (`_agree`) every rank reads the accumulated flag and, if any rank failed, ALL step down one mode together
    (captured -> split -> eager) and drop their graphs -- never a lasting mix of modes.  The captured step is the same launches on the same data: with the same random draws its
    parameters match the eager step's bit for bit (tests/test_gpu_step_graph.py).  Learning rate and Adam bias
    corrections are read from device memory refreshed before each replay; torch's device RNG advances per replay
    exactly as it does per eager step.  The capture runs the forward on fresh leaf aliases of the parameters and takes
    the gradients with autograd.grad, so autograd state that callers keep alive (a loss with history) cannot pull
    another stream into it.

    ema_decay / ema_warmup / max_grad_norm (all off by default: nothing above changes) go to optim.FusedAdam, which
    keeps an exponential moving average of the weights and clips the gradients by their global norm inside the fused
    update, in every launch mode (in a multi-rank run the norm is taken after the exchange, on the averaged gradients,
    so the replicas stay identical).  `grad_norm` is the last step's pre-clip norm as a 0-d device tensor (no sync);
    `with trainer.ema_weights(): drivers.evaluate(model, ...)` samples from the EMA.  The xgmi reducer applies Adam
    inside its own all-reduce kernel and has neither: VF_REDUCER=xgmi with either option raises ValueError.

    accum_steps = A (default 1: nothing above changes, launch for launch): step(batch) still takes the whole batch and
    performs ONE optimizer step, but runs the batch as A contiguous micro-batches (split_batch; B % A == 0) -- forward and
    backward on micro-batch m, then one launch that adds its gradient, weighted B_m / B, into FusedAdam's accumulators --
    and then the norm pass (max_grad_norm) and the Adam (+ EMA) launch on the accumulated gradient, which is also what
    p.grad shows afterwards.  Peak activation memory is one micro-batch's; the price is one more parameter-sized buffer.
    LR schedule, `it`, Adam's step count and the EMA advance once per step(); the returned loss is sum_m (B_m / B) loss_m,
    the full batch's loss, a device tensor.  With seed= micro-batch m draws for the ids the undivided batch gives its
    samples, so the accumulated gradient is the big batch's up to summation order.  In graph mode the geometry key is a
    MICRO-batch's geometry and a graph holds forward + backward + the accumulate launch ({beta, weight} read from device
    memory: the same graph serves every m and every later step); the norm and Adam launches follow the last replay
    eagerly, as in "split" mode.  GRAPH_AFTER / GRAPH_MAX count micro-batch sightings and `graph_steps` micro-batch
    replays.  The weight packs at the head of a micro-batch graph are repeated for m > 0 (profiles/grad_accum.md prices
    them).  Single process, GPU model only: world > 1 or a CPU model with accum_steps > 1 raises ValueError (the gradient
    arena averages in place as segments complete).

    loss_bins = K (default None: nothing above changes): the trainer owns a K-bin histogram of the per-sample loss by noise
    level -- two K-element device accumulators that the loss kernels add into (ViewFusion.loss_hist; csrc/loss_weight.h) --
    read with loss_by_level().  With it the loss-option kernels run even for the default objective (the same launch count).
    The objective itself is the model's: `model.set_loss(...)`; a set_loss() call between steps takes effect on the next
    step -- the captured steps are dropped and every geometry is captured again after its eager sightings -- never a
    replay of the old objective.  In graph mode the accumulators, `model.last_sample_loss` and
    `model.last_level` are static buffers of the captured step; with accum_steps > 1 every micro-batch adds its samples
    (B counts per step) and the two `last_*` tensors show the last micro-batch.  GPU model only.

    Conditioning dropout (`model.set_cond_dropout(p)`, classifier-free guidance; default 0: nothing above changes) is the
    model's too, and p is part of the same key: a change between steps drops the captured steps.  With seed= a sample's
    mask is a function of (seed, sample id) -- the same under accum_steps, graph replay and any split over ranks;
    `model.last_cond_drop` is a static buffer of the captured step (the last micro-batch's with accum_steps > 1).  An
    injected `cond_drop=` mask is a graph input, like the injected draws.

    Self-conditioning (`model.set_self_cond(p)`, csrc/diffusion.hip; default None: nothing above changes) is the model's
    as well, and p is part of the same key.  Its first pass -- the no-grad forward that makes the estimate
    (ViewFusion.self_cond_targets) -- runs launch by launch in front of every (micro-)step, in every launch mode, and
    hands the step `self_cond` (and, without seed=, the t / u / noise / cond_drop it drew) as injected inputs, which are
    graph inputs: a captured step holds the second pass alone.  With seed= a sample's coin is a function of (seed,
    sample id), the same under accum_steps and graph replay.  `model.last_self_cond` = (keep, x^) of the last first pass.
    Multi-rank: the phase has no collective; nothing else is built for it.

    A learned variance (`model.set_learned_variance(vlb_weight)`, csrc/diffusion.hip; default None: nothing above
    changes) is the model's as well, and the weight is part of the same key.  The hybrid step has the default step's
    launch count, so every launch mode, seed=, accum_steps, loss_bins, max_grad_norm and the EMA take it unchanged;
    in graph mode `model.last_sample_vlb` is a static buffer of the captured step, like `last_sample_loss`.

    Residual-block Dropout (`UNet(dropout=p)`) needs no argument here: with seed= every mask is a function of (seed,
    sample id, view index, layer, element) drawn inside the Dropout kernel and drawn again by its backward
    (ops.dropout_seeded).  The seed is a constant of the captured launches; the ids and the offsets table they read, in
    the forward and in the backward, are the graph's `sample_ids` input and its offsets buffer.  With accum_steps > 1
    each micro-batch keys its masks by its own slice of the ids, so they are the undivided batch's.  Without seed= the
    masks come from torch's device generator, as before.

    Noise-level sampling (`model.set_level_sampler(...)`, csrc/level_sampler.h; default None: nothing above changes) is the
    model's as well, and every call of it drops the captured steps.  Its three launches -- the table draw in place of the
    uniform one, the scaled loss finish, the statistics update -- are part of the captured step: the table, the
    statistics and the ready flag live in device memory that the sampler keeps for its whole life, so a replay draws from
    the table as the step before left it, and replay equals eager bit for bit.  `model.last_t` /
    `model.last_importance_weight` are static buffers of the captured step; level_proposal() reads the table.  With
    accum_steps > 1 every micro-batch draws from the table as it stands and then updates it, so later micro-batches of a
    step see an updated proposal: equality with the undivided batch is NOT claimed then (each micro-batch is still
    unbiased on its own).  Single process, GPU model only: world > 1 or a CPU model with a level sampler raises ValueError
    (the statistics would be rank-local and the ranks' proposals would drift apart; a reduction of them is not built).
    Checkpoints: drivers.save_checkpoint(..., level_sampler=model.level_sampler.state_dict()).

    Progressive distillation (`model.set_distill(teacher, steps=K)`, csrc/diffusion.hip; default None: nothing above
    changes) is the model's too, and every call of it drops the captured steps.  The teacher phase -- the draw of the
    student step, the teacher's two no-grad forwards and the two distillation kernels (ViewFusion.distill_targets) -- runs
    launch by launch in front of every step, and with accum_steps > 1 in front of every micro-batch (the draws are
    functions of the sample id, so a micro-batch targets what its samples target in the undivided batch); the student's
    step then takes z_t, its level, eps~ and x~ as injected inputs, which are graph inputs like t / u / noise.  A captured
    step therefore holds the student's launches only -- the capture's GroupNorm / convolution accounting and the primed
    tables are the student's, as before -- and replay equals eager bit for bit.  The optimizer holds the student's
    parameters only; the teacher never changes.  `model.last_distill` = (i, x~) of the last (micro-)batch.  Capturing
    the teacher phase as a graph of its own is not built (profiles/distill.md prices it).  GPU model only; a multi-rank
    run is not refused (the teacher phase has no collective) and not claimed."""
    GRAPH_AFTER = 2
    GRAPH_MAX = 96
    AGREE_EVERY = 64            # multi-rank agreement: the failure flag is read at least this often (see _agree)
    inject_capture_failure = None   # set by tests (class or instance attribute), never read from the environment

    def __init__(self, model, world=1, local_rank=0, lr_warmup=2500, decay_it=4000000, bucket_cap_mb=32, graph=None,
                 seed=None, global_batch=None, ema_decay=None, ema_warmup=False, max_grad_norm=None, accum_steps=1,
                 loss_bins=None):
        if isinstance(accum_steps, bool) or not isinstance(accum_steps, int) or accum_steps < 1:
            raise ValueError(f"accum_steps must be a positive integer, got {accum_steps!r}")
        if accum_steps > 1 and world > 1:
            raise ValueError("accum_steps > 1 is single-process only: the gradient exchange of a multi-rank run (every "
                             "reducer) averages each micro-batch's gradients as they complete, and holding the "
                             "collectives back until the last micro-batch is not built")
        if accum_steps > 1 and not next(model.parameters()).is_cuda:
            raise ValueError("accum_steps > 1 accumulates inside the fused HIP optimizer: the model must be on the GPU")
        self.accum_steps = accum_steps
        if loss_bins is not None:
            if isinstance(loss_bins, bool) or not isinstance(loss_bins, int) or loss_bins < 1:
                raise ValueError(f"loss_bins must be a positive integer or None, got {loss_bins!r}")
            if not next(model.parameters()).is_cuda:
                raise ValueError("loss_bins is filled by the fused HIP loss kernels: the model must be on the GPU")
            if not hasattr(model, "set_loss"):
                raise ValueError("loss_bins needs a ViewFusion model (its forward feeds the histogram)")
            dev = next(model.parameters()).device
            model.loss_hist = (torch.zeros(loss_bins, device=dev, dtype=torch.float32),
                               torch.zeros(loss_bins, device=dev, dtype=torch.int32))
        self.loss_bins = loss_bins
        self.module = model
        self.world = world
        self._check_level_sampler()
        # seed: the training draws come from the counter-based generator (csrc/rng.h) keyed by a global sample index
        # (step_sample_ids), not from torch's device generator; None (default): as before
        self.seed, self.global_batch = seed, global_batch
        self._ids = {}              # B -> (arange(B), this iteration's ids): device int64, rewritten in place per step
        self.model = model
        self.arena = None
        kind = os.environ.get("VF_REDUCER", "arena")
        extras = ema_decay is not None or max_grad_norm is not None
        if extras and kind == "xgmi":
            raise ValueError("VF_REDUCER=xgmi applies Adam inside its all-reduce kernel, which has neither the weight EMA "
                             "nor gradient clipping: use the default reducer (or VF_REDUCER=ddp) with ema_decay / "
                             "max_grad_norm")
        if extras and not next(model.parameters()).is_cuda:
            raise ValueError("ema_decay / max_grad_norm are part of the fused HIP Adam step: the model must be on the GPU")
        if world > 1 and kind != "ddp":
            try:
                # "xgmi": the hand-written one-shot all-reduce over IPC-mapped peer arenas fused with Adam (correctness-
                # only so far: it has run with two processes on one GPU, never across devices); default: RCCL
                self.arena = reducer.ACTIVE = (reducer.XgmiArena if kind == "xgmi" else reducer.GradArena)(model, world)
            except (RuntimeError, dist.DistBackendError) as e:    # first collective of the job (parameter broadcast)
                import traceback
                traceback.print_exc()    # (anything else -- a programming error in the hook set-up -- propagates as is)
                reducer.ACTIVE = None
                raise SystemExit(
                    f"[view_fusion_amd] gradient-arena set-up failed at world={world}: {type(e).__name__}: {e}\n"
                    "  -> relaunch (a fresh process group, not a re-exec) with VF_REDUCER=ddp to use torch's "
                    "DistributedDataParallel for the gradient exchange (VF_REDUCER=xgmi: first back to the default, "
                    "the arena over RCCL); see tools/scale_run.md") from e
        elif world > 1:
            kw = dict(broadcast_buffers=False, gradient_as_bucket_view=True, bucket_cap_mb=bucket_cap_mb)
            if next(model.parameters()).is_cuda:
                kw.update(device_ids=[local_rank], output_device=local_rank)
            self.model = DistributedDataParallel(model, **kw)
            # DDP copies a gradient into its bucket from a hook on the AccumulateGrad node, during the backward pass:
            # a GroupNorm gradient whose column sum is deferred to the end of the pass would be read before it exists
            for p in model.parameters():        # (per parameter, not a process-wide switch: other models keep deferring)
                p._vf_no_defer = True
        # modules whose behaviour depends on train/eval mode (see step()): the blocks that carry a Dropout
        self._mode_modules = [m for m in model.modules() if getattr(m, "dropout", 0) and hasattr(m, "_drop")]
        self.sched = LrScheduler(peak_lr=1e-4, peak_it=lr_warmup, decay_it=decay_it, decay_rate=0.16)
        self._named = list(model.named_parameters())
        params = self._params = [p for _, p in self._named]
        if params[0].is_cuda:       # one multi-tensor HIP launch per step
            from .optim import FusedAdam
            self.opt = FusedAdam(params, lr=self.sched.get_cur_lr(0), ema_decay=ema_decay, ema_warmup=ema_warmup,
                                 max_grad_norm=max_grad_norm)
        else:                       # CPU harness tests (gloo) only
            self.opt = torch.optim.Adam(params, lr=self.sched.get_cur_lr(0))
        self.it = -1
        if graph is None:
            graph = os.environ.get("VF_STEP_GRAPH", "1") == "1"
        # (with torch DDP the iteration stays eager: its reducer is driven by autograd hooks on the host)
        self.use_graph = bool(graph) and params[0].is_cuda and (world == 1 or self.arena is not None) and \
            not getattr(self.arena, "owns_optimizer_step", False)     # (the xgmi reducer: eager launches only)
        self._graph_wanted = self.use_graph     # what the run was configured for (a local capture failure clears use_graph)
        self._graphs = {}           # geometry key -> _StepGraph
        self._pool = None           # the graphs' shared private memory pool
        self._scal = None           # device {lr, 1-b1^t, 1-b2^t}
        self._last_graph = None
        self._loss_key = None       # ViewFusion.loss_key() the kept graphs were captured under
        self._graph_epoch = None    # FusedAdam.graph_epoch the kept graphs were captured under (None: none captured)
        self.graph_steps = 0        # iterations (accum_steps > 1: micro-batches) that ran as a replay (diagnostics / tests)
        self._check_base = self.GRAPH_AFTER     # multi-rank agreement: flag read at _check_base + 1, 4, 16, then every AGREE_EVERY
        self.demotions = 0

    @property
    def mode(self):
        """Launch mode of the iteration: "eager", "graph" (single process), "split" / "captured" (gradient arena)."""
        if not self.use_graph:
            return "eager"
        if self.arena is None:
            return "graph"
        return "captured" if self.arena.capturable else "split"

    @property
    def grad_norm(self):
        """Global L2 norm of the last step's (averaged) gradients before clipping: a 0-d device tensor that every
        step rewrites, never a sync.  None without max_grad_norm."""
        return getattr(self.opt, "grad_norm", None)

    def loss_by_level(self, reset=False):
        """-> (mean_loss (K,), count (K,) int32): the per-sample training loss by noise level since the last reset -- bin k
        holds the samples with min(K - 1, int(gamma K)) == k, gamma the sample's continuous level, so bin 0 is the noisiest.
        The loss is the UNWEIGHTED per-sample mean of the penalty (what `model.last_sample_loss` shows), so curves
        compare across weightings; a bin without samples gives NaN.  Device tensors, computed without a host sync:
        reading them is the caller's sync.  reset=True zeroes the accumulators afterwards (the sums are fp32: reset at
        every logging interval of a long run).  Rank-local under every reducer: each rank bins the samples it ran itself,
        and nothing is exchanged -- reduce the sums and counts across ranks yourself if you need the global curve."""
        if self.loss_bins is None:
            raise ValueError("loss_by_level needs Trainer(loss_bins=K)")
        bin_sum, bin_cnt = self.module.loss_hist
        mean, count = bin_sum / bin_cnt.to(torch.float32), bin_cnt.clone()
        if reset:
            bin_sum.zero_()
            bin_cnt.zero_()
        return mean, count

    def _check_level_sampler(self):
        if getattr(self.module, "_level_spec", None) is None:
            return
        if self.world > 1:
            raise ValueError("a level sampler is single-process only: its loss statistics are rank-local, so the ranks' "
                             "proposals would differ, and a reduction of them across ranks is not built")
        if not next(self.module.parameters()).is_cuda:
            raise ValueError("a level sampler draws and updates inside HIP kernels: the model must be on the GPU")

    def level_proposal(self):
        """-> (p (K,) float64, seen (K,) int32, ready (1,) bool) of the model's level sampler: the probability of each
        bin of timesteps as the table stands (the uniform n_k / (T - 1) while a "loss_aware" sampler is warming up), how
        many samples each bin's statistic has seen, and whether the table is in use.  Device tensors, computed without a
        host sync: reading them is the caller's sync."""
        smp = getattr(self.module, "level_sampler", None)
        if smp is None:
            raise ValueError("level_proposal needs model.set_level_sampler(...) on a GPU model")
        return smp.proposal()

    def ema_state_dict(self):
        return self.opt.ema_state_dict()

    def load_ema_state_dict(self, sd):
        self.opt.load_ema_state_dict(sd)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model holds the EMA weights (and the EMA tensors hold the live ones): one in-place
        exchange on entry, one on exit, after which the live weights are what they were, bit for bit.  The contents
        move, not the tensors -- captured graphs and packed weights address parameter memory by raw pointer -- and the
        parameters' version counters are bumped so the packed-weight caches refresh.  Do not call step() inside."""
        self.opt.swap_ema()
        try:
            yield self.module
        finally:
            self.opt.swap_ema()

    def dist_info(self):
        """What a multi-rank run looks like from this rank (bench.py prints it)."""
        info = dict(world_size=self.world, reducer="none" if self.world == 1 else (("xgmi" if getattr(self.arena, "owns_optimizer_step", False) else "arena") if self.arena else "ddp"),
                    launch_mode=self.mode, graph_steps=self.graph_steps, mode_demotions=self.demotions)
        if dist.is_available() and dist.is_initialized():
            info.update(world_size=dist.get_world_size(), rank=dist.get_rank(), backend=dist.get_backend())
            if info["backend"] == "nccl":
                try:
                    info["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
                except Exception:           # noqa: BLE001
                    info["rccl_version"] = None
        if self.arena is not None:
            info["gradients_copied_last_step"] = self.arena.copied
        return info

    def _drop_graphs(self):
        self._graphs, self._last_graph, self._pool, self._graph_epoch = {}, None, None, None

    def _agree(self):
        """Multi-rank agreement on the launch mode (see the class doc).  Called at the top of every step; reads the
        arena's accumulated failure flag (one host sync) only at the iteration numbers below."""
        a = self.arena
        if a is None or a.flag_acc is None:
            return
        # d = 1, 4, 16 after the last change of mode (a capture that fails does so at a geometry's first capture, i.e.
        # early), then every AGREE_EVERY-th iteration for the rest of the run: a geometry first met at iteration 1000, or a
        # run whose `it` was restored from a checkpoint, is never more than AGREE_EVERY iterations away from the next
        # check (one host sync per 64 iterations).  Every rank computes the same iteration numbers.
        d = self.it - self._check_base
        if d < 1 or not (d in (1, 4, 16) or d % self.AGREE_EVERY == 0):
            return
        if float(a.flag_acc.item()) == 0.0:        # the same averaged value on every rank
            return
        was = "captured" if a.capturable and self._graph_wanted else ("split" if self._graph_wanted else "eager")
        if was == "captured":
            a.capturable = False
            self.use_graph = True
        else:
            self.use_graph = self._graph_wanted = False
        import sys
        print(f"[view_fusion_amd] rank {dist.get_rank() if dist.is_initialized() else 0}: a training-step capture failed "
              f"on some rank; all ranks step down from '{was}' to '{self.mode}' at iteration {self.it}", file=sys.stderr)
        self._drop_graphs()
        a.flag_value = 0.0
        a.flag_acc.zero_()
        self._check_base = self.it
        self.demotions += 1

    # -- whole-step HIP graph ---------------------------------------------------------------------------------------
    def _graph_key(self, batch, extra):
        from . import ops
        if not self.use_graph or ops.st.KERNEL_LOG is not None or (self.arena is not None and self.arena.flat is None):
            return None
        # injected draws are graph inputs, and so are the sample ids of the seeded draws and the teacher phase's outputs of a
        # distillation step; the seed is a constant of the captured launches, so it is part of the key; nothing else is
        if any(k not in ("t", "u", "noise", "seed", "sample_ids", "self_cond", "cond_drop") + DISTILL_INPUTS for k in extra):
            return None
        seed = extra.get("seed")
        extra = {k: v for k, v in extra.items() if k != "seed" and v is not None}
        vc = batch["view_count"]
        if torch.is_tensor(vc):
            if vc.is_cuda:          # reading it back would be a device sync per step
                return None
            vc = vc.tolist()
        ts = [("y_0", batch["y_0"]), ("y_cond", batch["y_cond"]), ("angle", batch["angle"])] + sorted(extra.items())
        if not all(torch.is_tensor(t) and t.is_cuda for _, t in ts):
            return None
        vc = tuple(int(v) for v in vc)
        if len(vc) != batch["y_0"].shape[0] or min(vc) < 1 or max(vc) > batch["y_cond"].shape[1]:
            return None                       # the eager path raises the reference's errors
        # the launch geometry depends on the stacked-view count S only: WHICH sample owns which views is the offsets
        # table the kernels read from device memory, a graph input like the images
        # (+ the addresses of what a captured step reads besides its inputs and is replaceable from outside: the noise
        # schedule buffer -- set_new_noise_schedule() makes new tensors -- and the parameter storage)
        g = getattr(self.module, "gammas", None)
        anchors = (g.data_ptr() if torch.is_tensor(g) else 0, self._params[0].data_ptr(), self._params[-1].data_ptr())
        return tuple((k, tuple(t.shape), t.dtype) for k, t in ts) + (anchors + (seed,), sum(vc)), vc

    def _capture(self, e, key, vc, batch, extra, accum=False):
        from . import ops
        dev = batch["y_0"].device
        arena = self.arena
        inj = self.inject_capture_failure    # tests only: "<rank>:<mode>" fails that rank's captures in that mode
        if inj and dist.is_initialized() and inj == f"{dist.get_rank()}:{self.mode}":
            raise RuntimeError("injected capture failure (Trainer.inject_capture_failure)")
        # With a host-driven transport (gloo) the graph ends with the backward pass; the exchange and the Adam launch
        # follow each replay eagerly.  On RCCL the segment all-reduces and Adam are part of the graph.
        # A micro-batch of an accumulated step (accum): the graph ends with the accumulate launch instead; the norm
        # and Adam launches follow the last micro-batch's replay eagerly.
        split = accum or (arena is not None and not arena.capturable)
        adam = None if split else self.opt.graph_begin()
        if adam is None and not split:
            return False
        acc = self.opt.accum_begin() if accum else None
        if accum and acc is None:
            return False
        if self._scal is None:
            self._scal = torch.zeros(3, device=dev, dtype=torch.float32)
        e.inputs = {k: {**batch, **extra}[k].detach().clone().contiguous() for k, _, _ in key[:-2]}
        e.view_count = torch.tensor(vc, dtype=torch.int64, device=dev)
        offs = ops.view_offsets(e.view_count, dev)   # resolved (one read-back) and remembered BEFORE the capture
        e.off, e.vc = offs[0], vc                    # the offsets table: rewritten when a replay's view_count differs
        tables = ops.prime_tables(getattr(self.module, "denoise_fn", None), key[-1], dev, tuple(batch["y_0"].shape[-2:]))
        self.opt.zero_grad()                           # the capture allocates the gradients in the graph's pool
        g = torch.cuda.CUDAGraph()
        kw = {} if self._pool is None else dict(pool=self._pool)
        ops.begin_capture(dev, sum(1 for m in self.module.modules() if isinstance(m, torch.nn.GroupNorm)),
                          sum(1 for m in self.module.modules() if isinstance(m, torch.nn.Conv2d)))
        failed = None
        try:
            with torch.cuda.graph(g, capture_error_mode="relaxed", **kw):
                try:        # an exception must not unwind through the capture: let it end, then report
                    # The captured forward runs on FRESH leaf tensors that alias the parameters' storage
                    # (functional_call), and its gradients are taken with autograd.grad: nothing passes through the
                    # parameters' own AccumulateGrad nodes.  Those remember the stream they were created on; if a
                    # caller keeps ANY tensor with autograd history of this model alive (a loss from an earlier
                    # forward), they are bound to the default stream, the backward pass forks the capture onto it, and
                    # hipStreamEndCapture takes the process down.
                    leaves = {n: p.detach().requires_grad_(True) for n, p in self._named}
                    if arena is not None:              # gradients are born in (or moved into) the all-reduce buffer
                        arena.capture_begin(list(leaves.values()))
                    seeded = {} if extra.get("seed") is None else dict(seed=extra["seed"])
                    loss = torch.func.functional_call(self.model, leaves, (),
                                                      dict(view_count=e.view_count, **e.inputs, **seeded))
                    grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
                    if arena is not None:
                        grads = arena.capture_finish(grads)
                    for (_, p), gr in zip(self._named, grads):
                        p.grad = gr
                    if acc is not None:
                        self.opt.accumulate_captured(acc)
                    elif not split:
                        self.opt.step_captured(adam, self._scal)
                except Exception as err:      # noqa: BLE001
                    failed = err
        finally:
            fix = ops.end_capture()
        if failed is not None:
            if arena is not None:
                arena.capture_abort()
            raise failed
        if self._pool is None:
            self._pool = g.pool()
        e.adam = None if split else self.opt.graph_end(adam)
        e.accum = None if acc is None else self.opt.accum_end(acc)
        self._graph_epoch = self.opt.graph_epoch if split else adam["epoch"]
        e.loss, e.graph = loss.detach(), g
        # the loss-option kernels' per-sample outputs are static buffers of this graph (None on the default path)
        e.sample = None
        if getattr(self.module, "_loss", None) is not None or getattr(self.module, "loss_hist", None) is not None or \
                getattr(self.module, "_level_spec", None) is not None or \
                getattr(self.module, "_lv_weight", None) is not None:
            e.sample = (self.module.last_sample_loss, self.module.last_level)
        e.vlb = getattr(self.module, "last_sample_vlb", None)      # a learned variance: the step's per-sample vlb, likewise
        e.drop = getattr(self.module, "last_cond_drop", None)      # conditioning dropout: the step's mask, likewise
        e.level = (getattr(self.module, "last_t", None), getattr(self.module, "last_importance_weight", None))
        e.grads = list(grads)
        # what the captured launches address besides the graph's own pool
        e.keep = (fix, tables, offs, getattr(self.module, "gammas", None))
        return True

    def _graph_step(self, e, vc, batch, extra, accum=None):
        if vc != e.vc:
            off = [0]
            for v in vc:
                off.append(off[-1] + v)
            e.off.copy_(torch.tensor(off, dtype=torch.int32).pin_memory(), non_blocking=True)
            e.vc = vc
        for k, dst in e.inputs.items():
            src = extra[k] if k in extra else batch[k]
            dst.copy_(src.reshape(dst.shape), non_blocking=True)
        if e.sample is not None:
            self.module.last_sample_loss, self.module.last_level = e.sample
        if hasattr(self.module, "last_cond_drop"):
            self.module.last_cond_drop = e.drop
        if e.vlb is not None:
            self.module.last_sample_vlb = e.vlb
        if hasattr(self.module, "last_t"):             # the level sampler's draw: static buffers of the graph, likewise
            self.module.last_t, self.module.last_importance_weight = e.level
        if accum is not None:                          # a micro-batch: its gradient goes into the accumulators, which
            self.opt.accum_tick(e.accum, *accum)       # the optimizer step after the last one reads and leaves in .grad
            e.graph.replay()
            self.graph_steps += 1
            return e.loss.clone()
        if self._last_graph is not e:                  # .grad shows the gradients of the graph that ran last
            for p, gr in zip(self._params, e.grads):
                p.grad = gr
            self._last_graph = e
        if e.adam is None:                             # host-driven transport: exchange + Adam follow the replay
            e.graph.replay()
            self.arena.reduce_all()
            self.opt.step()
        else:
            self.opt.graph_tick(e.adam, self._scal)
            e.graph.replay()
        self.graph_steps += 1
        return e.loss.clone()

    def _step_ids(self, batch):
        """This iteration's sample ids, written (one launch, no host buffer) into the per-B device tensor."""
        B, dev = batch["y_0"].shape[0], batch["y_0"].device
        ent = self._ids.get(B)
        if ent is None:
            ent = self._ids[B] = (torch.arange(B, dtype=torch.int64, device=dev),
                                  torch.empty(B, dtype=torch.int64, device=dev))
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        torch.add(ent[0], step_sample_ids(self.it, B, rank, self.world, self.global_batch), out=ent[1])
        return ent[1]

    def draw_batch(self, store, B, max_views=6, relative=False):
        """The batch of the step about to run, assembled from a data.ViewStore in one launch: its sample ids are
        step_sample_ids(self.it + 1, B, rank, world, global_batch) + b -- the very ids that step's t / u / noise draws
        use -- so `trainer.step(trainer.draw_batch(store, 16))` is the whole training loop body, and a sample's views,
        view_count and object are functions of (seed, id) like its noise: unchanged by accum_steps, by the launch mode
        and by how the global batch is split over ranks (every rank holds the store; the ids are disjoint by
        construction).  Needs Trainer(seed=...).  No host sync."""
        if self.seed is None:
            raise ValueError("draw_batch draws from the seeded generator: construct the Trainer with seed=...")
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        first = step_sample_ids(self.it + 1, B, rank, self.world, self.global_batch)
        ent = self._ids.get(("draw", B))
        if ent is None:
            ent = self._ids[("draw", B)] = (torch.arange(B, dtype=torch.int64, device=store.device),
                                            torch.empty(B, dtype=torch.int64, device=store.device))
        torch.add(ent[0], first, out=ent[1])
        return store.batch(self.seed, torch.arange(first, first + B, dtype=torch.int64), mode="train",
                           max_views=max_views, relative=relative, ids_device=ent[1])

    def step(self, batch, **extra):
        """One reference iteration; returns the (device) loss tensor, no host sync."""
        self.it += 1
        if self.seed is not None and "seed" not in extra:
            extra = dict(extra, seed=self.seed)
            if extra.get("sample_ids") is None:
                extra["sample_ids"] = self._step_ids(batch)
        lr = self.sched.get_cur_lr(self.it)
        for gparam in self.opt.param_groups:
            gparam["lr"] = lr
        # The reference calls model.train() every iteration (experiment.py:286); Module.train() walks all ~1400
        # submodules (2 ms), so it runs only when some module that HAS a mode-dependent layer is not in training mode.
        # The residual blocks' Dropout is the only such layer; the root flag alone would miss `vf.denoise_fn.eval()`.
        if not self.model.training or any(not m.training for m in self._mode_modules):
            self.model.train()
        self._agree()
        if self.accum_steps == 1:
            return self._run(batch, extra)
        w, total = 1.0 / self.accum_steps, None
        for m, (bm, em) in enumerate(split_batch(batch, extra, self.accum_steps)):
            part = self._run(bm, em, accum=(w, m == 0)) * w
            total = part if total is None else total + part
        self.opt.step()                                # the norm pass and Adam (+ EMA) on the accumulated gradient
        return total

    def _run(self, batch, extra, accum=None):
        """Forward, backward and the optimizer step on `batch` as a replay or launch by launch; accum = (weight, first):
        `batch` is a micro-batch, and in place of the optimizer step its gradient is added into the accumulators."""
        loss_key = getattr(self.module, "loss_key", None)
        loss_key = None if loss_key is None else loss_key()
        if loss_key != self._loss_key:
            # the objective (model.set_loss), the histogram or the conditioning-dropout probability changed: all are
            # constants of the captured launches, so
            # the captured steps are dropped (and their memory freed); every geometry is captured again after its eager
            # sightings.  A replay never keeps the old objective.
            if self._graphs:
                self._drop_graphs()
            self._loss_key = loss_key
            self._check_level_sampler()
        if getattr(self.module, "_distill", None) is not None and "distill_z" not in extra:
            # progressive distillation: the teacher phase of this (micro-)batch, no-grad and launch by launch, in front of
            # the student's step, which takes its four outputs as injected inputs (graph inputs of a captured step) --
            # so a capture holds the student's launches alone, and its accounting is the default step's
            draws = {k: extra[k] for k in ("t", "noise", "seed", "sample_ids") if extra.get(k) is not None}
            tgt = self.module.distill_targets(batch["y_cond"], batch["view_count"], batch["angle"], batch["y_0"], **draws)
            extra = {**{k: v for k, v in extra.items() if k not in ("t", "u", "noise")}, **tgt}
        if getattr(self.module, "self_cond", None) is not None and "self_cond" not in extra:
            # self-conditioning: the first pass of this (micro-)batch, no-grad and launch by launch, in front of the step,
            # which takes the estimate (and, unseeded, the draws the pass used) as injected inputs -- so a capture holds
            # the second pass alone, and its accounting is the default step's
            draws = {k: extra[k] for k in ("t", "u", "noise", "cond_drop", "seed", "sample_ids") if extra.get(k) is not None}
            first = self.module.self_cond_targets(batch["y_cond"], batch["view_count"], batch["angle"], batch["y_0"],
                                                  **draws)
            extra = {**extra, **first}
        key, vc = self._graph_key(batch, extra) or (None, None)
        if key is not None and accum is None and self._graph_epoch is not None and \
                self.opt.graph_epoch != self._graph_epoch:      # (a micro-batch graph addresses no Adam state)
            # the optimizer state was replaced (load_state_dict, a changed parameter set): the captured steps still
            # address the old moment tensors -- drop them; every geometry is captured again after its eager sightings
            self._drop_graphs()
        if key is not None:
            e = self._graphs.get(key)
            if e is None and len(self._graphs) < self.GRAPH_MAX:
                e = self._graphs[key] = _StepGraph()
            if e is not None:
                if e.graph is None and e.seen >= self.GRAPH_AFTER:
                    try:
                        if not self._capture(e, key, vc, batch, extra, accum=accum is not None):
                            self.use_graph = False
                            if self.arena is not None:     # this rank stays eager: tell the others (as a failure does)
                                self.arena.flag_value = 1.0
                    except Exception as err:           # leave the run on the eager path, loudly
                        import sys
                        print(f"[view_fusion_amd] training-step graph capture failed ({type(err).__name__}: {err}); "
                              "continuing eagerly" + ("" if self.arena is None else
                                                      " and telling the other ranks (failure flag)"), file=sys.stderr)
                        self.use_graph, e.graph = False, None
                        if self.arena is not None:     # rides the next gradient all-reduce; every rank steps down at
                            self.arena.flag_value = 1.0    # the next agreement point (_agree)
                        self.opt.zero_grad()
                if e.graph is not None:
                    return self._graph_step(e, vc, batch, extra, accum)
                e.seen += 1
        self._last_graph = None
        self.opt.zero_grad()
        fused = self.arena is not None and getattr(self.arena, "owns_optimizer_step", False)
        if fused:                         # the exchange kernels apply Adam themselves (reducer.XgmiArena)
            self.arena.begin_step(self.opt)
        loss = self.model(y_0=batch["y_0"], y_cond=batch["y_cond"], view_count=batch["view_count"],
                          angle=batch["angle"], **extra)
        loss.backward()
        if self.arena is not None:
            self.arena.finish()
        if accum is not None:
            self.opt.accumulate(*accum)
        elif not fused:
            self.opt.step()
        # detached: a caller that keeps the returned loss should not keep this iteration's autograd graph (its saved
        # activations: several GB at B=16) alive with it
        return loss.detach()
