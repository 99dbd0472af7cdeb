"""The callers either side of the hot path that SURVEY §8(f) lists as "next" rows, restated for the
MI355X engine (no dataset / wandb / image-grid plumbing):

  * sampler drivers with the reference's real call shapes ... experiment.py:472-488 (extrapolate,
    7..23 conditioning views), :516-544 (autoregressive 24-step rollout, view_count 1 -> 24),
    :580-599 (weight animation: B=24 target angles x N=6 views in one call)
  * checkpoint wire format ................................. utils/checkpoint.py:31-72
  * eval reduction: PSNR, SSIM + all_reduce(AVG) + barriers  utils/metrics.py:6-12, utils/dist.py:69-91,
    experiment.py:314-370 (SSIM is the metric the reference selects best_model_ssim.pt by, :375-380)
  * LPIPS (vgg), the third number of the paper's tables ..... utils/compute_metrics.py (the user brings the weights)
"""
import contextlib
import math
import os
import re

import torch
import torch.distributed as dist


@contextlib.contextmanager
def _eval_mode(model):
    """The reference's eval / inference entry points call `self.model.eval()` first (experiment.py:316): Dropout (the
    only mode-dependent layer of the UNet) must be off while sampling.  The previous mode is restored on exit, so a
    Trainer that finds the model in training mode keeps skipping its (slow) Module.train() walk."""
    was = model.training
    if was:
        model.eval()
    try:
        yield
    finally:
        if was:
            model.train()


# ---- sampler drivers ---------------------------------------------------------------------------
# Each driver reaches the sampler through model(..., generate=True), like the reference's (DDP wraps forward), and
# takes the optional injected randomness of ViewFusion.forward (y_t = the start noise, z_seq[i] = the noise of
# reverse step i) so that its output can be compared with the CPU oracle.  seed= (and sample_ids=) reach generate() the
# same way: the draws then come from the counter-based generator of csrc/rng.h, keyed per sample.  So do sample_steps= /
# solver= / eta= (few-step sampling: K steps over a sub-sequence of the trained schedule instead of all T) and guidance=
# (classifier-free guidance: a scale, or one per sample; ViewFusion.generate), and with it threshold= / threshold_max= /
# guidance_rescale= (dynamic thresholding of y0_hat, the guided noise rescaled; ViewFusion.generate).
@torch.no_grad()
def extrapolate(model, cond, angle, max_views=6, view_count=None, generator=None, **inject):
    """Generate with MORE views than the model was trained on (view_count ~ U[max_views+1, 24)),
    experiment.py:472-488.
    cond (B,23,3,H,W), angle (B,1) -> (generated_batch (B,1+k,3,H,W), logit_arr, weight_arr, view_count).
    **inject reaches generate(): y_t, z_seq, seed, sample_ids, use_graph, sample_steps / solver / eta for a
    few-step chain, guidance (a classifier-free guidance scale, or one per sample), threshold / threshold_max /
    guidance_rescale and variance ("analytic") (ViewFusion.generate)."""
    B = cond.shape[0]
    if view_count is None:
        view_count = torch.randint(max_views + 1, 24, (B,), generator=generator)
    with _eval_mode(model):
        _, ret, logit_arr, weight_arr, _ = model(y_cond=cond, view_count=view_count, angle=angle, generate=True,
                                                 **inject)
    return ret.clamp(0, 1), logit_arr, weight_arr, view_count


@torch.no_grad()
def autoregressive_rollout(model, first_view, steps=24, y_t=None, z_seq=None, seed=None, sample_ids=None,
                           sample_steps=None, solver="ddim", eta=0.0, guidance=None, threshold=None,
                           threshold_max=None, guidance_rescale=None, variance=None):
    """Start from ONE view and synthesise the orbit view by view, feeding every sample back as an
    extra conditioning view (count = 1 .. steps; angle = 2*pi/24 * count), experiment.py:516-544.
    first_view (B,3,H,W) -> samples (B,steps,3,H,W).  y_t / z_seq: per-count lists of injected randomness.
    seed: the draws of rollout step `count` of object b use the id sample_ids[b] * steps + count - 1 (sample_ids
    defaults to arange(B)), so every step of every object has noise of its own, independent of the batch.
    sample_steps / solver / eta: the few-step sampler of every generate() call (`steps` is the rollout length).
    guidance: the classifier-free guidance scale of every generate() call (a number, or one per object).
    threshold / threshold_max / guidance_rescale: likewise, of every generate() call (ViewFusion.generate).
    variance: likewise ("analytic": the analytic variance of the model's moments, ViewFusion.generate)."""
    cond = first_view[:, None].contiguous()
    B = cond.shape[0]
    out = []
    if seed is not None:
        base = torch.arange(B) if sample_ids is None else torch.as_tensor(sample_ids).reshape(-1).cpu()
        base = (base.to(torch.int64) * steps).to(cond.device)
    with _eval_mode(model):
        for count in range(1, steps + 1):
            view_count = torch.full((B,), count)
            angle = torch.full((B, 1), 2 * math.pi / 24 * count, device=cond.device)
            inject = dict(y_t=None if y_t is None else y_t[count - 1],
                          z_seq=None if z_seq is None else z_seq[count - 1])
            if seed is not None:
                inject.update(seed=seed, sample_ids=base + (count - 1))
            if sample_steps is not None:
                inject.update(sample_steps=sample_steps, solver=solver, eta=eta)
            if guidance is not None:
                inject.update(guidance=guidance)
            for name, val in (("threshold", threshold), ("threshold_max", threshold_max),
                              ("guidance_rescale", guidance_rescale), ("variance", variance)):
                if val is not None:
                    inject[name] = val
            *_, sample = model(y_cond=cond, view_count=view_count, angle=angle, generate=True, **inject)
            cond = torch.cat((cond, sample[:, None]), dim=1)
            out.append(sample)
    return torch.stack(out, dim=1)


@torch.no_grad()
def orbit_frames(model, all_views, n=24, **inject):
    """The weight-animation ("GIF") call shape, experiment.py:580-599: ONE object's `all_views` (24,3,H,W); every one
    of the n target angles 2*pi/n*i is generated from the same 6 conditioning views (every 4th view), i.e. one
    generate() call at B = n, N = 6.
    -> (generated_batch (n,1+k,3,H,W) clamped to [0,1], logit_arr, weight_arr, cond_views (n,6,3,H,W), angles (n,1));
    the frame i of the animation shows weight_arr[i] next to cond_views[i] and generated_batch[i].
    **inject reaches generate() (sample_steps / solver / eta among it: 24 frames in K instead of T steps; guidance: a
    classifier-free guidance scale, or one per frame; threshold / threshold_max / guidance_rescale with it)."""
    assert all_views.shape[0] == 24 and n % 24 == 0
    dev = all_views.device
    angles = torch.tensor([2 * math.pi / n * i for i in range(n)], dtype=torch.float32, device=dev).unsqueeze(1)
    target = torch.repeat_interleave(all_views, n // 24, dim=0)
    cond_views = torch.stack([all_views[::4]] * target.shape[0], dim=0).contiguous()
    view_count = torch.full((target.shape[0],), cond_views.shape[1])
    with _eval_mode(model):
        _, ret, logit_arr, weight_arr, _ = model(y_cond=cond_views, view_count=view_count, angle=angles, generate=True,
                                                 **inject)
    return ret.clamp(0, 1), logit_arr, weight_arr, cond_views, angles


# ---- checkpoint wire format --------------------------------------------------------------------
def _check_distill_extra(d):
    k = d.get("steps") if isinstance(d, dict) else None
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"the checkpoint's distill entry must be dict(steps=K) with an integer K >= 1, got {d!r}")


def save_checkpoint(path, model, optimizer, **extra):
    """{"model": state_dict, "optimizer": state_dict, + extra (it, t, run_id, ssim, psnr)} -- the
    reference's file layout, so either side can load the other's checkpoints.  distill=dict(steps=K) records the stage of
    a progressive distillation (load_checkpoint); the teacher's weights are not part of the file.
    self_cond=model.self_cond records the self-conditioning setting, which state_dict() does not hold (only the stem's
    shape differs); learned_variance=model.learned_variance likewise records the vlb weight of a learned variance (only
    the head's shape differs).  moments=estimate_moments(...) (or a (T,) tensor: the model's own prediction is recorded
    with it) records the per-level moments of the analytic variance, which state_dict() does not hold either; the file
    gets {"moment" (T,) float64, "prediction", optionally "count"}."""
    out = dict(extra)
    if out.get("distill") is not None:
        _check_distill_extra(out["distill"])
    if out.get("moments") is not None:
        m = out["moments"]
        m = dict(m) if isinstance(m, dict) else dict(moment=m)
        m["moment"] = torch.as_tensor(m["moment"]).detach().to(device="cpu", dtype=torch.float64).reshape(-1).clone()
        m.setdefault("prediction", getattr(model, "prediction", "eps"))
        out["moments"] = m
    out["model"] = model.state_dict()
    out["optimizer"] = optimizer.state_dict()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(out, path)


def load_checkpoint(path, model, optimizer=None, device=None):
    """Loads "model" (and "optimizer" if given and present); returns the remaining entries.
    An "ema" entry (save_checkpoint(..., ema=trainer.ema_state_dict())) is restored into an optimizer that keeps a
    weight EMA (optim.FusedAdam(ema_decay=...)) and, like every extra entry, also returned.  A "level_sampler" entry
    (save_checkpoint(..., level_sampler=model.level_sampler.state_dict())) is restored into a model that has had the same
    set_level_sampler(...) call: the statistics and the proposal table continue where they were.  A "prediction" entry
    (save_checkpoint(..., prediction=model.prediction)) must name the model's own prediction: ValueError otherwise,
    before anything is loaded.  A "distill" entry (save_checkpoint(..., distill=dict(steps=K)): the stage of a progressive
    distillation the weights were saved in -- the model samples in K steps, and its next stage is K / 2 with these weights
    as the teacher) is a plain dict with an integer steps >= 1, checked (ValueError otherwise) and returned with the other
    extras: the caller builds the teacher and calls set_distill.  A "self_cond" entry (save_checkpoint(...,
    self_cond=model.self_cond): the self-conditioning probability, or None) must equal the model's own: ValueError
    otherwise, before anything is loaded.  A "learned_variance" entry (save_checkpoint(...,
    learned_variance=model.learned_variance): the vlb weight, or None) likewise.  A "moments" entry
    (save_checkpoint(..., moments=...): the per-level moments of the analytic variance) must have been recorded for the
    model's own prediction and number of timesteps: ValueError otherwise, before anything is loaded; it is handed back
    with the other extras -- the caller calls model.set_moments(extras["moments"]).  Files without the entry load as
    before."""
    sd = torch.load(path, map_location=device, weights_only=False)
    if sd.get("distill") is not None:
        _check_distill_extra(sd["distill"])
    mine = getattr(model, "prediction", "eps")
    if sd.get("prediction") is not None and sd["prediction"] != mine:
        raise ValueError(f"the checkpoint was trained with prediction {sd['prediction']!r}, the model is set to {mine!r} "
                         "(set_prediction)")
    if "self_cond" in sd and sd["self_cond"] != getattr(model, "self_cond", None):
        raise ValueError(f"the checkpoint was trained with self-conditioning {sd['self_cond']!r}, the model is set to "
                         f"{getattr(model, 'self_cond', None)!r} (set_self_cond)")
    if "learned_variance" in sd and sd["learned_variance"] != getattr(model, "learned_variance", None):
        raise ValueError(f"the checkpoint was trained with a learned variance of vlb weight {sd['learned_variance']!r}, the "
                         f"model is set to {getattr(model, 'learned_variance', None)!r} (set_learned_variance)")
    if sd.get("moments") is not None:
        m = sd["moments"]
        if not isinstance(m, dict) or "moment" not in m:
            raise ValueError("the checkpoint's moments entry must be dict(moment=(T,), prediction=...)")
        if m.get("prediction", mine) != mine:
            raise ValueError(f"the checkpoint's moments were recorded for prediction {m.get('prediction')!r}, the model is "
                             f"set to {mine!r}: the noise estimate differs")
        T = getattr(model, "num_timesteps", None)
        if T is not None and torch.as_tensor(m["moment"]).numel() != T:
            raise ValueError(f"the checkpoint's moments hold {torch.as_tensor(m['moment']).numel()} levels, the model's "
                             f"schedule {T}")
    model.load_state_dict(sd["model"])
    if optimizer is not None and "optimizer" in sd and sd["optimizer"].get("state"):
        optimizer.load_state_dict(sd["optimizer"])
    if sd.get("ema") and getattr(optimizer, "ema_decay", None) is not None:
        optimizer.load_ema_state_dict(sd["ema"])
    if sd.get("level_sampler") and getattr(model, "level_sampler", None) is not None:
        model.level_sampler.load_state_dict(sd["level_sampler"])
    return {k: v for k, v in sd.items() if k not in ("model", "optimizer")}


# ---- progressive distillation -----------------------------------------------------------------
def progressive_distill(trainer, teacher, batches, start_steps, end_steps, iters_per_stage, guidance=None,
                        from_ema=False):
    """Salimans & Ho's outer loop around ViewFusion.set_distill (csrc/diffusion.hip holds the definition): for
    K = start_steps / 2, start_steps / 4, ..., end_steps the trainer's model is trained for `iters_per_stage` steps as a
    K-step student of the 2K-step `teacher`, then its parameters are copied INTO the teacher (copy_: no tensor is
    replaced, so packed-weight caches refresh and nothing is reallocated) -- the student's EMA instead when the trainer
    keeps one and from_ema=True -- and K halves.  guidance applies to the first stage only: from the second stage on the
    teacher is a distilled student, which needs no null row.  batches: an iterator of trainer.step() batches (at least
    stages x iters_per_stage of them).  start_steps = end_steps 2^m with m >= 1 and start_steps <= T, else ValueError.
    -> [(K, mean loss of the stage as a 0-d device tensor)]; no host sync.  Distillation stays set (at the last K) on
    return: model.set_distill(None) goes back to the plain objective."""
    model = trainer.module
    for name, v in (("start_steps", start_steps), ("end_steps", end_steps), ("iters_per_stage", iters_per_stage)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    ratio = start_steps // end_steps
    if start_steps % end_steps or ratio < 2 or ratio & (ratio - 1):
        raise ValueError(f"start_steps must be end_steps times a power of two (at least 2): got {start_steps} and {end_steps}")
    if start_steps > model.num_timesteps:
        raise ValueError(f"start_steps must be at most T = {model.num_timesteps}, got {start_steps}")
    if from_ema and getattr(trainer.opt, "ema_decay", None) is None:
        raise ValueError("from_ema=True needs a Trainer that keeps a weight EMA (ema_decay=...)")
    batches = iter(batches)
    student = dict(model.named_parameters())
    out, K = [], start_steps // 2
    while K >= end_steps:
        model.set_distill(teacher, steps=K, guidance=guidance)
        total = None
        for _ in range(iters_per_stage):
            loss = trainer.step(next(batches))
            total = loss if total is None else total + loss
        out.append((K, total / iters_per_stage))
        with torch.no_grad():
            for name, p in teacher.named_parameters():
                src = student[name]
                p.copy_(trainer.opt._ema_of(src) if from_ema else src)
        guidance = None
        K //= 2
    return out


# ---- eval reduction -----------------------------------------------------------------------------
def compute_psnr(generated, target):
    """20*log10(1/sqrt(mse)) per image; the per-image mean of squared differences is one HIP launch."""
    from . import ops
    return ops.psnr(generated, target)


def compute_ssim(generated, target):
    """pytorch_msssim.ssim(generated, target, data_range=1.0, size_average=False) per image (utils/metrics.py:11-12)
    as our own kernel: two HIP launches, no third-party package."""
    from . import ops
    return ops.ssim(generated, target, data_range=1.0)


# torchvision's index of the 13 convolutions inside vgg16().features, and their widths
_VGG_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
_VGG_KEY = re.compile(r"^(?:net\.slice\d+\.|features\.)?(\d+)\.(weight|bias)$")


class LPIPS(torch.nn.Module):
    """lpips.LPIPS(net="vgg") (version 0.1) for eval: the VGG16 trunk as 13 frozen nn.Conv2d holders (`features.N`, N =
    torchvision's index) and the five bias-free 1x1 "lin" layers as (1,C,1,1) parameters `lin0` ... `lin4`.  No weights
    ship with the package: build it from the two state dicts the user already has, move it to the
    device, and call it -- or hand it to evaluate(lpips=...) -- with images in [0, 1]."""

    def __init__(self):
        super().__init__()
        from .ops import LPIPS_TAPS, LPIPS_WIDTHS
        convs, cin = {}, 3
        for idx, cout in zip(_VGG_CONVS, LPIPS_WIDTHS):
            convs[str(idx)] = torch.nn.Conv2d(cin, cout, 3, padding=1)
            cin = cout
        self.features = torch.nn.ModuleDict(convs)
        for l, i in enumerate(LPIPS_TAPS):
            self.register_parameter(f"lin{l}", torch.nn.Parameter(torch.zeros(1, LPIPS_WIDTHS[i], 1, 1)))
        self.requires_grad_(False)

    @property
    def convs(self):
        return [self.features[str(i)] for i in _VGG_CONVS]

    @property
    def lins(self):
        return [getattr(self, f"lin{l}") for l in range(5)]

    @classmethod
    def from_state_dicts(cls, vgg_sd, lin_sd):
        """vgg_sd: torchvision vgg16 keys `features.N.{weight,bias}` (also `N.…` or the package's `net.sliceK.N.…`);
        lin_sd: the package's `lin{0..4}.model.1.weight` of shape (1,C,1,1).  Every shape is checked; the first missing
        or mis-shaped key is named."""
        net = cls()
        found = {}
        for k, v in vgg_sd.items():
            m = _VGG_KEY.match(k)
            if m and int(m.group(1)) in _VGG_CONVS:
                found[f"features.{m.group(1)}.{m.group(2)}"] = (k, v)
        own = {}
        for name, p in net.named_parameters():
            if name.startswith("features."):
                src = found.get(name)
                shown = src[0] if src is not None else name
                val = src[1] if src is not None else None
            else:
                shown = f"{name}.model.1.weight"
                val = lin_sd.get(shown)
            if val is None:
                raise KeyError(f"LPIPS: missing key {shown!r}")
            if not torch.is_tensor(val) or tuple(val.shape) != tuple(p.shape):
                raise ValueError(f"LPIPS: key {shown!r} has shape {tuple(getattr(val, 'shape', ()))}, expected "
                                 f"{tuple(p.shape)}")
            own[name] = val.detach().to(torch.float32)
        net.load_state_dict(own)
        return net

    @classmethod
    def from_files(cls, vgg_path, lin_path):
        return cls.from_state_dicts(torch.load(vgg_path, map_location="cpu", weights_only=True),
                                    torch.load(lin_path, map_location="cpu", weights_only=True))

    @torch.no_grad()
    def forward(self, generated, target):
        from . import ops
        return ops.lpips(generated, target, self)


def compute_lpips(generated, target, net):
    """lpips.LPIPS(net="vgg")(2 * generated - 1, 2 * target - 1) per image pair, (B,): `net` is an LPIPS module on the
    images' device.  The trunk runs on the engine's conv kernels, the rest in csrc/lpips.hip."""
    from . import ops
    return ops.lpips(generated, target, net)


def reduce_dict(d, average=True):
    """all_reduce every tensor of `d` across ranks (AVG by default), keys in sorted order as the reference
    (utils/dist.py:69-91); identity without a process group.  RCCL has ncclAvg; gloo only SUM, so there the mean is
    SUM / world."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() < 2:
        return d
    native_avg = dist.get_backend() == "nccl"
    out = {}
    for k in sorted(d):
        v = d[k].clone()
        if average and native_avg:
            dist.all_reduce(v, op=dist.ReduceOp.AVG)
        else:
            dist.all_reduce(v, op=dist.ReduceOp.SUM)
            if average:
                v /= dist.get_world_size()
        out[k] = v
    return out


def _barrier():
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()


@torch.no_grad()
def evaluate(model, batches, max_views=6, generator=None, extra_metrics=None, ssim=False, seed=None, lpips=None,
             guidance=None, threshold=None, threshold_max=None, guidance_rescale=None, nll=False, **inject):
    """The eval reduction of Experiment.eval (experiment.py:314-370): every rank generates its shard of the validation
    batches (view_count ~ U[1, max_views] per sample), PSNR per image on the GPU (utils/metrics.py:6-8), mean over the
    rank's images, barrier, all_reduce(AVG) of the scalars, barrier.  `batches`: iterable of dicts with target (B,3,H,W),
    cond (B,>=max_views,3,H,W), angle (B,1) and optionally view_count.  ssim=True adds the reference's second metric
    (utils/metrics.py:11-12, images of at least 11 x 11) under "ssim", through the same reduction; the default reports
    PSNR alone.  lpips=<an LPIPS module on the device> adds "lpips" (images a multiple of 16 and at least 32 a side) the
    same way.  extra_metrics: {name: fn(generated, target) -> (B,)} for anything else (merged on top).  Returns the
    reduced dict of 0-d tensors.
    seed (default None: torch's device generator, as before): the sampler's noise comes from the counter-based generator
    keyed by batch["ids"] (B,) -- dataset indices -- so an image's sample, and with it the metrics, do not depend on how
    the validation set is batched or sharded over ranks.  Without "ids" a running index over this rank's images is
    used: independent of the batch size, but NOT of the sharding.
    sample_steps / solver / eta (through **inject): evaluate with a K-step sampler (ViewFusion.generate); which K is
    good enough for a checkpoint is what this function measures.
    guidance (default None: the unguided sampler): a classifier-free guidance scale for every generate() call -- which
    scale suits a checkpoint trained with set_cond_dropout is, likewise, what this function measures.
    threshold / threshold_max / guidance_rescale (default None: off): dynamic thresholding and guidance rescaling of
    every generate() call (ViewFusion.generate) -- what keeps a sweep over g > 1 from measuring saturation alone.
    nll=True (default False: today's launches and keys) adds "bpd", the variational bound of the targets in bits per
    dimension on the full T-step chain (ViewFusion.bound_terms with the batch's view_count, seed and ids; bits_per_dim
    below has the options and the per-step curves), through the same reduction.  ValueError together with guidance /
    threshold / guidance_rescale (a guided model's "bound" is no bound) and for a model bound_terms refuses (a
    self-conditioned or a CPU model), before the first generate() launches anything."""
    if nll and (guidance is not None or threshold is not None or (guidance_rescale is not None and
                                                                  float(guidance_rescale) > 0)):
        raise ValueError("evaluate(nll=True) takes no guidance / threshold / guidance_rescale: the bound is that of the "
                         "conditional model's own reverse process")
    core = getattr(model, "module", model)
    bpd = []
    if nll:                                        # what bound_terms refuses is refused here, before the first generate()
        core._check_bound(core.gammas.device)
    if guidance is not None:
        inject = dict(inject, guidance=guidance)
    for name, val in (("threshold", threshold), ("threshold_max", threshold_max), ("guidance_rescale", guidance_rescale)):
        if val is not None:
            inject[name] = val
    gen, gt = [], []
    seen = 0
    with _eval_mode(model):                        # Experiment.eval: self.model.eval() (experiment.py:316)
        for b in batches:
            vc = b.get("view_count")
            if vc is None:
                vc = torch.randint(1, max_views + 1, (b["target"].shape[0],), generator=generator)
            n = b["target"].shape[0]
            if seed is not None:
                ids = b.get("ids")
                if ids is None:
                    ids = torch.arange(seen, seen + n)
                inject = dict(inject, seed=seed, sample_ids=ids)
            seen += n
            *_, samples = model(y_cond=b["cond"], view_count=vc, angle=b["angle"], generate=True, **inject)
            gen.append(samples)
            gt.append(b["target"])
            if nll:
                bpd.append(core.bound_terms(b["cond"], vc, b["angle"], b["target"], seed=seed,
                                            sample_ids=inject.get("sample_ids") if seed is not None else None)["total_bpd"])
    _barrier()
    metrics = {"psnr": compute_psnr}
    if ssim:
        metrics["ssim"] = compute_ssim                 # module global, looked up now: a host stand-in can be patched in
    if lpips is not None:
        metrics["lpips"] = lambda a, t: compute_lpips(a, t, lpips)     # (a module global too, looked up at call time)
    metrics.update(extra_metrics or {})
    out = {k: torch.cat([fn(a, t) for a, t in zip(gen, gt)]).mean() for k, fn in metrics.items()}
    if nll:
        out["bpd"] = torch.cat(bpd).mean()
    _barrier()
    out = reduce_dict(out)
    _barrier()
    return out


@torch.no_grad()
def bits_per_dim(model, batches, seed=None, sample_steps=None, clip_denoised=True, fixed_variance="small"):
    """The variational bound of held-out targets in bits per dimension (Improved DDPM's calc_bpd_loop on this engine):
    every rank runs ViewFusion.bound_terms on its shard of `batches` -- the dicts of evaluate(): target (B,3,H,W), in the
    model's own range [-1, 1], cond, angle and optionally view_count (default: every view of cond) and ids -- then mean
    over the rank's images, barrier, all_reduce(AVG), barrier, as evaluate().  Returns the reduced dict {"bpd", "prior_bpd":
    0-d tensors; "vb", "x0_mse", "eps_mse": (K,) curves over the steps of the chain}: vb[k] is the term of step k (the
    decoder at k = 0), x0_mse / eps_mse the error of the recovered image / noise at that level -- the validation curve.
    seed (default None: torch's device generator): the noisy targets come from the counter-based generator keyed by
    batch["ids"] (kind 6, csrc/rng.h), so an image's terms do not depend on how the set is batched or sharded; without
    "ids" a running index over this rank's images is used, as in evaluate().
    sample_steps (default None: all T steps): the bound of the K-step stochastic chain -- what a strided chain loses.
    clip_denoised / fixed_variance: ViewFusion.bound_terms."""
    core = getattr(model, "module", model)
    keys = ("total_bpd", "prior_bpd", "vb", "x0_mse", "eps_mse")
    got = {k: [] for k in keys}
    seen = 0
    for b in batches:
        n = b["target"].shape[0]
        vc = b.get("view_count")
        if vc is None:
            vc = [b["cond"].shape[1]] * n
        ids = None
        if seed is not None:
            ids = b.get("ids")
            if ids is None:
                ids = torch.arange(seen, seen + n)
        seen += n
        terms = core.bound_terms(b["cond"], vc, b["angle"], b["target"], seed=seed, sample_ids=ids,
                                 sample_steps=sample_steps, clip_denoised=clip_denoised, fixed_variance=fixed_variance)
        for k in keys:
            got[k].append(terms[k])
    _barrier()
    out = {("bpd" if k == "total_bpd" else k): torch.cat(v).mean(dim=0) for k, v in got.items()}
    _barrier()
    out = reduce_dict(out)
    _barrier()
    return out


@torch.no_grad()
def estimate_moments(model, batches, seed=None, levels=None):
    """The statistic of the analytic variance (Analytic-DPM): M[t] = E |eps_hat(y_t)|^2 / d of the model's noise estimate,
    per trained level, by Monte Carlo -- every rank runs ViewFusion.eps_moments on its shard of `batches` (the dicts of
    bits_per_dim: target (B,3,H,W) in the model's own range, cond, angle, optionally view_count and ids), one draw per
    (image, level); the per-sample moments are summed in float64 on the host side, after the loop (one sync per batch),
    and sums and counts are all-reduced over the ranks.  Returns {"moment": (T,) float64 CPU tensor, NaN where no level
    was visited; "count": (T,) int64 CPU tensor, the draws behind each level; "prediction": the model's}: hand it to
    model.set_moments and to save_checkpoint(..., moments=).
    seed (default None: torch's device generator): the noisy targets come from the counter-based generator keyed by
    batch["ids"] (kind 6, the bound's: use another seed than for the bound on the same images), so an image's moments
    do not depend on how the set is batched or sharded.
    levels (default None: all T): K evenly strided levels or an explicit sequence (schedule.sample_timesteps) -- a chain
    needs the moments of its own levels only, optimal_trajectory those of every level it may choose."""
    core = getattr(model, "module", model)
    T = core.num_timesteps
    total = torch.zeros(T, dtype=torch.float64)
    count = torch.zeros(T, dtype=torch.int64)
    seen = 0
    for b in batches:
        n = b["target"].shape[0]
        vc = b.get("view_count")
        if vc is None:
            vc = [b["cond"].shape[1]] * n
        ids = None
        if seed is not None:
            ids = b.get("ids")
            if ids is None:
                ids = torch.arange(seen, seen + n)
        seen += n
        got = core.eps_moments(b["cond"], vc, b["angle"], b["target"], seed=seed, sample_ids=ids, levels=levels)
        tau = got["tau"].cpu()
        total[tau] += got["m2"].double().sum(dim=0).cpu()
        count[tau] += n
    _barrier()
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dev = core.gammas.device
        both = torch.cat([total, count.double()]).to(dev)
        dist.all_reduce(both)
        both = both.cpu()
        total, count = both[:T], both[T:].round().to(torch.int64)
    _barrier()
    moment = torch.where(count > 0, total / count.clamp_min(1).double(), torch.full_like(total, float("nan")))
    return {"moment": moment, "count": count, "prediction": core.prediction}
