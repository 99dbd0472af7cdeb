"""MI355X-native ViewFusion: host-side mirror of the reference `ViewFusion` module.

Same constructor, `set_new_noise_schedule`, `forward(y_cond, view_count, angle, y_0=None,
noise=None, generate=False)`, `generate`, `p_sample`, `p_mean_variance`, `q_sample`,
`predict_start_from_noise`, `q_posterior` and the same six persistent schedule buffers as
/root/reference/model/view_fusion.py:12-300 -- so `state_dict()` is interchangeable.

What differs is underneath: the ragged view stacking + q_sample, the softmax-over-views
compose + MSE (and its backward) and the reverse-step tail are single fused HIP kernels driven
by a device prefix-sum of `view_count`; nothing on the path calls `.tolist()` / `.item()` when
`view_count` is handed over as a CPU tensor or list (as the reference's training loop does).

Extras (default None = reference behaviour): `forward(..., t=, u=)` and
`generate(..., z_seq=)` / `forward(generate=True, y_t=, z_seq=)` inject the random draws so that
runs -- also the sampler drivers, which reach generate() through forward() as the reference's
do -- can be compared against the CPU oracle; `sample()` is an alias of `generate()`.

`seed=` (with optional `sample_ids=`, default arange(B)) on `forward` / `generate` takes every draw that was not
injected from the counter-based generator of csrc/rng.h instead of torch's device generator: a draw is then a function
of (seed, sample id, purpose, step, element) alone -- the same for a sample whatever its row, its batch or its rank --
and tests/rng_ref.py can restate it on the CPU.

`set_loss(...)` (default: the reference's unweighted MSE, untouched) selects the training objective's penalty (mse / l1 /
huber) and a per-sample weight of the noise level (min-SNR, P2); see csrc/loss_weight.h.

Classifier-free guidance (csrc/diffusion.hip holds the definition; both halves off by default, and then every path runs
the launches it ran before): `set_cond_dropout(p)` zeroes the conditioning views of a training sample with probability
p, and `generate(..., guidance=g)` (also `forward(generate=True)`, `p_sample`, `p_mean_variance`) runs one unconditional
row per sample next to the conditional ones and extrapolates the noise prediction, g eps_c + (1 - g) eps_u.
`threshold=q` (optional `threshold_max=c`) and `guidance_rescale=phi` on the same four entry points are the two remedies
for what g > 1 does to a pixel-space sample: dynamic thresholding of y0_hat (clamp to the per-sample q-quantile of
|y0_hat|, then divide by it) in place of the static clamp, and the guided noise rescaled to the conditional one's
standard deviation.  Both off by default; both defined at the head of csrc/diffusion.hip.

`set_level_sampler(...)` (default None: uniform timesteps, every launch as before) draws a training sample's timestep
from a proposal over bins of timesteps -- a fixed one, or one that follows the loss's second moment per bin -- and
multiplies the sample's loss by the importance weight that keeps the objective unbiased; see csrc/level_sampler.h.

`set_prediction("eps" | "v" | "x0")` (default "eps": the launches and the bits of before) says what the network's first
three channels mean: the noise, v = sqrt(g) noise - sqrt(1 - g) y_0, or y_0 itself.  Training forms the target inside
the loss kernels; sampling hands every reverse-step tail the (a, b) pair of y0_hat = a y - b out that belongs to the
prediction, so generate() and everything built on it need no new argument.  csrc/diffusion.hip holds the definition.

`set_distill(teacher, steps=K)` (default None: every launch and every bit as before) turns the training forward into one
step of progressive distillation (Salimans & Ho): the target is what the frozen `teacher` -- another ViewFusion, held
outside the module tree -- reaches in two deterministic DDIM steps of its 2K-step chain, and the model learns to get
there in one step of its own K-step chain.  csrc/diffusion.hip holds the definition; drivers.progressive_distill halves K.

`set_self_cond(p)` (default None: every launch and every bit as before) shows the network -- built with three more input
channels -- its own previous estimate of the clean image: in training the estimate of one extra no-grad forward, kept
with probability p; in sampling the y0 the previous reverse step computed anyway.  csrc/diffusion.hip holds the definition.

`set_learned_variance(vlb_weight)` (default None: every launch and every bit as before) trains a network built with three
more output channels to predict, per pixel, the log-variance of a reverse step between log beta~ and log beta (Improved
DDPM): forward() takes L_simple + vlb_weight L_vlb in the same launch count, and the stochastic few-step sampler (ddim,
eta = 1) draws its noise at that scale.  csrc/diffusion.hip holds the definition, csrc/vlb.h the arithmetic.
"""
import torch
from torch import nn

from . import schedule as _schedule


class ViewFusion(nn.Module):
    def __init__(self, denoise_fn, beta_schedule, weighting_train=True, weighting_inference=True, **kwargs):
        super().__init__(**kwargs)
        self.denoise_fn = denoise_fn
        self.beta_schedule = beta_schedule
        self.weighting_train = weighting_train
        self.weighting_inference = weighting_inference
        # the training objective (set_loss) and what the optional loss kernels hand back: plain attributes, no buffers
        self._loss = None                 # None: the reference's unweighted MSE through compose_mse_loss
        self.loss_hist = None             # (bin_sum, bin_cnt) device accumulators, attached by train.Trainer(loss_bins=)
        self.last_sample_loss = self.last_level = None
        # conditioning dropout (set_cond_dropout) and the mask of the last training forward: plain attributes too
        self._cond_drop_p = 0.0
        self.last_cond_drop = None
        # noise-level sampling (set_level_sampler): the settings, the device state (ops.LevelSampler; GPU models only) and
        # the last training forward's draw: plain attributes too
        self._level_spec = None
        self._level_gen = 0
        self.level_sampler = None
        self.last_t = self.last_importance_weight = None
        # what the network predicts (set_prediction): a plain attribute too; the (a, b) tables of v / x0, made on demand
        self.prediction = "eps"
        self._pred_tabs = None
        # progressive distillation (set_distill): the settings -- the teacher among them, which is NOT a submodule -- and
        # the last training forward's (i, x~): plain attributes too
        object.__setattr__(self, "_distill", None)
        self._distill_gen = 0
        self.last_distill = None
        # self-conditioning (set_self_cond): the probability p (None: off) and the last training forward's (keep, x^):
        # plain attributes too
        self._self_cond_p = None
        self.last_self_cond = None
        # a learned variance (set_learned_variance): the vlb weight (None: off), the last training forward's per-sample
        # vlb and the device tables (c1, hi, lo), made on demand: plain attributes too
        self._lv_weight = None
        self.last_sample_vlb = None
        self._lv_tabs = None
        # the analytic variance (set_moments): the per-level second moment of the noise estimate, float64 on the host
        # (None: not set), and a counter the cached plans key on: plain attributes too
        self._moments = None
        self._moments_gen = 0

    # -- the analytic variance ----------------------------------------------------------------
    def set_moments(self, moments=None):
        """The per-level second moment of this model's noise estimate, M[t] = E |eps_hat(y_t)|^2 / d: (T,) values
        (drivers.estimate_moments' "moment"; NaN where a level was not estimated), or None, the default: not set.
        What generate(variance="analytic") and bound_terms(fixed_variance="analytic") build the Analytic-DPM optimal
        variance from (schedule.analytic_sigma2; csrc/diffusion.hip holds the definition).  A plain attribute
        (`moments` reads it back, a float64 CPU tensor): no buffer, no parameter, state_dict() is unchanged -- save it as
        save_checkpoint(..., moments=...).  They are the moments of the model as it is now -- its weights, its
        prediction, its schedule -- and of the unguided model; nothing checks that.  ValueError for anything but one
        value per trained level."""
        self._moments_gen += 1
        if moments is None:
            self._moments = None
            return
        if isinstance(moments, dict):
            moments = moments["moment"]
        m = torch.as_tensor(moments).detach().to(device="cpu", dtype=torch.float64).reshape(-1).clone()
        T = getattr(self, "num_timesteps", None)
        if T is not None and m.numel() != T:
            raise ValueError(f"moments must hold one value per trained level ({T}), got {m.numel()}")
        self._moments = m

    @property
    def moments(self):
        """The moments of set_moments (float64 CPU tensor (T,)), None while they are not set."""
        return self._moments

    def _check_analytic(self, dev, what):
        """ValueError, before any launch, where the analytic variance cannot be used (`what` names the caller)."""
        if self._lv_weight is not None:
            raise ValueError(f"{what} on a model with a learned variance: the model has its own (DESIGN 8)")
        if self._moments is None:
            raise ValueError(f"{what} needs the model's moments: drivers.estimate_moments, then set_moments (DESIGN 8)")
        if self._moments.numel() != self.num_timesteps:
            raise ValueError(f"the moments hold {self._moments.numel()} levels, the schedule {self.num_timesteps}")
        if torch.device(dev).type != "cuda" or self.gammas.device.type != "cuda":
            raise ValueError(f"{what} runs on the GPU only (its reverse step and its terms are HIP kernels): move the "
                             "model and the batch there")

    # -- a learned variance -------------------------------------------------------------------
    def set_learned_variance(self, vlb_weight=1e-3):
        """A learned reverse-process variance (Nichol & Dhariwal, "Improved DDPM"; csrc/diffusion.hip holds the definition).
        set_learned_variance(None), the default: off -- every launch and every bit as before.

        The network -- UNet(out_channel=9) -- also predicts, in channels 6..8, where between log beta~ and log beta the
        log-variance of a reverse step lies, per pixel.  Training: forward() takes the hybrid objective L_simple +
        vlb_weight L_vlb -- L_simple is today's objective with every set_loss / set_prediction / loss_bins option, L_vlb
        the KL of the step's posterior from the model's Gaussian, in bits per dimension, with the mean held constant -- in
        the same launch count; `last_sample_vlb` (B,) is the per-sample vlb of the last training forward (a device tensor,
        no sync).  Sampling: generate() with solver "ddim" and eta = 1 -- which is what sample_steps=None runs, as
        sample_steps=T -- draws every step's noise at the learned per-pixel scale; every other (solver, eta) has no
        posterior-variance noise to replace and runs the existing kernels, which ignore channels 6..8.  p_sample takes the
        learned step, p_mean_variance returns the per-pixel log-variance, and the logits handed back are channels 3..5.
        A plain attribute (`learned_variance` reads it back): no buffer, no parameter -- save it as
        save_checkpoint(..., learned_variance=model.learned_variance).  A Trainer drops its captured steps when it changes.
        Refused with ValueError: together with set_distill (on either model), set_self_cond or a level sampler;
        threshold= / guidance_rescale=; and, when it runs, a CPU model or a network whose output is not 9 channels."""
        if vlb_weight is None:
            self._lv_weight = None
            self.last_sample_vlb = None
            return
        import math
        w = float(vlb_weight)
        if not math.isfinite(w) or w < 0:
            raise ValueError(f"the vlb weight must be finite and >= 0, got {vlb_weight}")
        if self._distill is not None:
            raise ValueError("a learned variance on a distillation student is not built (DESIGN 8): set_distill(None) first")
        if self._self_cond_p is not None:
            raise ValueError("a learned variance together with self-conditioning is not built (DESIGN 8): "
                             "set_self_cond(None) first")
        if self._level_spec is not None:
            raise ValueError("a learned variance together with a level sampler is not built (DESIGN 8): "
                             "set_level_sampler(None) first")
        self._lv_weight = w

    @property
    def learned_variance(self):
        """The vlb weight of set_learned_variance, None while it is off."""
        return self._lv_weight

    @staticmethod
    def _out_channels(net):
        last = None
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                last = m
        return None if last is None else last.out_channels

    def _check_lv(self, dev, threshold=None, guidance_rescale=None):
        """ValueError, before any launch, where a learned-variance pass cannot run."""
        if self._distill is not None or self._self_cond_p is not None or self._level_spec is not None:
            raise ValueError("a learned variance with distillation, self-conditioning or a level sampler is not built "
                             "(DESIGN 8)")
        if threshold is not None or (guidance_rescale is not None and float(guidance_rescale) > 0):
            raise ValueError("threshold= / guidance_rescale= with a learned variance are not built (DESIGN 8): the tails on "
                             "the eps buffer carry no variance")
        have = self._out_channels(self.denoise_fn)
        if have is not None and have != 9:
            raise ValueError(f"a learned-variance model reads 3 prediction + 3 logit + 3 variance channels = 9, the "
                             f"network gives out_channel = {have}")
        if torch.device(dev).type != "cuda":
            raise ValueError("a learned variance runs on the GPU only (its loss and its reverse step are HIP kernels): "
                             "move the model and the batch there")

    def _lv_tables(self):
        """The device tables of the hybrid loss on the full schedule: (posterior_mean_coef1, hi, lo), fp32 (T,)."""
        dev = self.gammas.device
        if self._lv_tabs is None or self._lv_tabs[0] != dev:
            hi, lo = _schedule.variance_tables(self.betas64)
            self._lv_tabs = (dev, torch.tensor(hi, dtype=torch.float32, device=dev),
                             torch.tensor(lo, dtype=torch.float32, device=dev))
        return self.posterior_mean_coef1, self._lv_tabs[1], self._lv_tabs[2]

    def _lv_plan(self, tau, dev):
        """The "ddim", eta = 1 plan of a chain with its variance tables (hi, lo) next to it."""
        plan = self._sampler_plan(tau, "ddim", 1.0, dev)
        if "hi" not in plan:
            hi, lo = _schedule.variance_tables(self.betas64, tau)
            plan["hi"] = torch.tensor(hi, dtype=torch.float32, device=dev)
            plan["lo"] = torch.tensor(lo, dtype=torch.float32, device=dev)
        return plan

    def _logits(self, out, S):
        """The view logits handed back: channels 3.. of the S conditional rows, 3..5 on a learned-variance model."""
        return out[:S, 3:6, ...] if self._lv_weight is not None else out[:S, 3:, ...]

    # -- training objective -------------------------------------------------------------------
    def set_loss(self, penalty="mse", delta=1.0, weighting=None, snr_gamma=5.0, p2_k=1.0, p2_gamma=1.0):
        """The training objective of forward(): loss = mean_b w_b mean_i rho(noise_hat - noise)  (csrc/loss_weight.h).

        penalty: "mse" (d^2), "l1" (|d|) or "huber" (F.huber_loss with `delta`).
        weighting: None (w = 1), "min_snr" (w = min(SNR, snr_gamma) / SNR, Hang et al.), "p2" (w = (p2_k + SNR)^-p2_gamma,
        Choi et al.) or "trunc_snr" (w = max(SNR, 1) / SNR: the truncated-SNR weight max(SNR, 1) on the x-space error of
        Salimans & Ho, which keeps a signal at low SNR for a distilled eps-student), with SNR = gamma / (1 - gamma) of the
        sample's own level.  No renormalisation by sum w.
        The defaults ARE the reference's loss, and with them forward() runs exactly the launches it ran before.  Anything
        else runs the loss-option kernels (the same launch count) and forward() then also leaves `last_sample_loss`
        (B,), the unweighted per-sample loss, and `last_level` (B,): detached device tensors, valid until the next
        forward.  Stores no parameter or buffer.  A Trainer drops its captured steps when these settings change."""
        from .ops.diffusion import PENALTIES, WEIGHT_KINDS
        if penalty not in PENALTIES:
            raise ValueError(f"unknown penalty {penalty!r}: one of {sorted(PENALTIES)}")
        if weighting not in WEIGHT_KINDS:
            raise ValueError(f"unknown loss weighting {weighting!r}: one of None, 'min_snr', 'p2', 'trunc_snr'")
        delta, snr_gamma, p2_k, p2_gamma = float(delta), float(snr_gamma), float(p2_k), float(p2_gamma)
        if not delta > 0:
            raise ValueError(f"delta must be positive, got {delta}")
        if not snr_gamma > 0:
            raise ValueError(f"snr_gamma must be positive, got {snr_gamma}")
        if not p2_k >= 0:
            raise ValueError(f"p2_k must be non-negative, got {p2_k}")
        if p2_gamma != p2_gamma:
            raise ValueError("p2_gamma must be a number")
        kind = None if weighting in (None, "none") else weighting
        a, b = (snr_gamma, 0.0) if kind == "min_snr" else ((p2_k, p2_gamma) if kind == "p2" else (0.0, 0.0))
        if penalty == "mse" and kind is None:
            self._loss = None
        else:
            self._loss = dict(penalty=penalty, delta=delta if penalty == "huber" else 1.0, weight_kind=kind, a=a, b=b)

    def set_cond_dropout(self, p=0.0):
        """Conditioning dropout for classifier-free guidance: in training mode, forward() replaces the conditioning
        views of a sample by zeros with probability p (the null conditioning that generate(guidance=) samples with).  A
        dropped sample keeps its view_count -- all its rows get the zero conditioning half -- so no shape changes.
        With seed= the draw is a function of (seed, sample id) alone (ops.draw_cond_drop); without, torch.rand(B) < p
        drawn after t, u and the noise.  forward(cond_drop=mask) injects the mask instead.  `last_cond_drop` is the
        mask of the last training forward (device uint8 (B,), None while the feature is off).  p = 0 (the default): off,
        the launches of before.  Stores no parameter or buffer; a Trainer drops its captured steps when p changes."""
        p = float(p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"the conditioning-dropout probability must be in [0, 1], got {p}")
        self._cond_drop_p = p

    def set_level_sampler(self, kind=None, bins=None, probs=None, ema=0.9, warmup=10, uniform_mix=0.01):
        """How forward() draws a training sample's timestep when `t` is not injected (csrc/level_sampler.h).

        kind None (the default): uniform on [1, T - 1], the launches and the bits of before; removes a sampler.
        "fixed": bin k of `bins` equal bins of timesteps is drawn with probability proportional to probs[k] (K masses,
        non-negative, not all zero; normalised on the host) -- emphasise a band of noise levels by hand.
        "loss_aware": bin k is drawn in proportion to n_k sqrt(m_k), m_k an exponential moving average (factor `ema` per
        update, default 0.9) of (w_b s_b)^2 over the samples that fell into the bin -- the loss-second-moment resampler of
        Improved DDPM with one EMA per bin in place of the paper's ten-loss history per timestep.  Until every bin has
        seen `warmup` samples (default 10, the paper's history length) the draw is the uniform one, bit for bit.
        bins (default min(64, T - 1); at most min(T - 1, 1024)).  uniform_mix (default 0.01): the share eps of the uniform
        proposal mixed in, p_k = (1 - eps) q_k / sum q + eps n_k / (T - 1); it bounds the importance weight by 1 / eps and
        must be at least 2 (T - 1) / 2^32.
        Every sample's loss is multiplied by its importance weight (T - 1)^-1 / P(t), so the expected gradient is the
        uniform objective's; this runs the loss-option kernels (ops.compose_loss) even with set_loss() at its default, plus,
        for "loss_aware" in training mode, one one-workgroup statistics launch after the loss.  An injected `t` bypasses
        the sampler entirely: no weight, no update.  `last_t` / `last_importance_weight` are the last sampled forward's
        draw (device tensors, no sync; None otherwise).  The state (`level_sampler`, an ops.LevelSampler with
        state_dict() / load_state_dict()) is a plain attribute: no parameter, no buffer.  Needs the noise schedule
        (set_new_noise_schedule) and, to run, a GPU model.  A Trainer drops its captured steps when this is called."""
        from . import ops
        if kind is not None and self._self_cond_p is not None:
            raise ValueError("a level sampler together with self-conditioning is not built (DESIGN 8): "
                             "set_self_cond(None) first")
        if kind is not None and self._lv_weight is not None:
            raise ValueError("a level sampler together with a learned variance is not built (DESIGN 8): "
                             "set_learned_variance(None) first")
        self._level_gen += 1
        if kind is None:
            self._level_spec = self.level_sampler = None
            return
        T = getattr(self, "num_timesteps", None)
        if T is None:
            raise ValueError("set_level_sampler needs the noise schedule: call set_new_noise_schedule first")
        if bins is None:
            bins = min(64, T - 1)
        K, probs, ema, warmup, uniform_mix = ops.check_level_sampler(kind, T, bins, probs, ema, warmup, uniform_mix)
        self._level_spec = dict(kind=kind, bins=K, probs=probs, ema=ema, warmup=warmup, uniform_mix=uniform_mix)
        dev = self.gammas.device
        self.level_sampler = ops.LevelSampler(kind, T, dev, **{k: v for k, v in self._level_spec.items() if k != "kind"}) \
            if dev.type == "cuda" else None

    def set_prediction(self, prediction="eps"):
        """What channels 0..2 of the network mean (csrc/diffusion.hip holds the definition; the weights: loss_weight.h).

        "eps" (the default): the noise -- every launch and every bit as before.
        "v": sqrt(g) noise - sqrt(1 - g) y_0, g the level the network is conditioned on.  "x0": y_0 itself.
        Training: forward() takes the loss on the network's own target, formed inside the loss kernels from the noise and
        y_0 it already holds (ops.compose_loss(prediction=): the same launch count, no target buffer); set_loss's
        penalties apply to that residual, weighting=None is w = 1 on it, and "min_snr" / "p2" stay weights on the
        eps-equivalent squared error (native weight w_eps(g) c(g), c = g for v and g / (1 - g) for x0).
        Sampling: generate / p_sample / p_mean_variance, ancestral or few-step, guided, thresholded or not, run the same
        tails with the prediction's table pair for y0_hat = a y - b out; guidance_rescale takes sigma of the composed
        output in the network's own parameterisation.  On a zero-terminal-SNR schedule (beta_schedule
        zero_terminal_snr=True) "v" and "x0" sample, "eps" raises ValueError.
        A plain attribute: no buffer, no parameter, state_dict() unchanged -- save it as
        save_checkpoint(..., prediction=model.prediction); load_checkpoint refuses a file that names another one.  A
        Trainer drops its captured steps when it changes.  Not built: switching the parameterisation of trained weights."""
        from .schedule import check_prediction
        self.prediction = check_prediction(prediction)
        self._pred_tabs = None
        self._plan = None

    def set_distill(self, teacher=None, steps=None, guidance=None, threshold=None, guidance_rescale=None):
        """Progressive distillation (Salimans & Ho; csrc/diffusion.hip holds the definition).  set_distill(None), the default:
        off -- every launch and every bit as before.

        teacher: another ViewFusion on the same device with the same noise schedule (betas and T), image channels and
        `relative` configuration; its `prediction` and `weighting_inference` are its own.  steps = K: the model becomes a
        K-step student of the teacher's 2K-step deterministic DDIM chain, 1 <= K <= T // 2.  In training mode forward()
        then draws a student step i in [0, K) per sample (seeded: mulhi32(word 0, K), the word that gives t otherwise;
        unseeded: torch.randint(0, K) where t is drawn; an injected t= is read as i), forms z_t at the level
        gammas[tau_S[i]] its own sample_steps=K sampler will use, runs the teacher's steps 2i+1 and 2i from there under
        no_grad, and takes the existing objective -- set_loss penalties and weights, loss_bins, last_sample_loss, last_level
        -- with noise := eps~ and y_0 := x~, the target that makes one student step land where the teacher's two do.
        guidance (a scale, or one per sample): the teacher's steps are guided (one null row per sample), so the student
        needs no null row at sampling time.  threshold / guidance_rescale of the teacher are not built: ValueError.
        The teacher is held outside the module tree: state_dict(), parameters(), modules(), the optimizer, DDP and
        functional_call never see it; it is put into eval mode, runs the UNet's inference path and its parameters get no
        gradient.  `last_distill` = (i, x~) of the last distillation forward (device tensors, no sync).
        Refused with ValueError: a level sampler, conditioning dropout p > 0 and, when forward() runs, a CPU
        model (the settings can be made on one, like a level sampler's).  A Trainer drops its captured steps when this is
        called and runs the teacher phase in front of every (micro-)step."""
        self._distill_gen += 1
        self.last_distill = None
        if teacher is None:
            if steps is not None or guidance is not None:
                raise ValueError("set_distill(None) turns distillation off: steps= / guidance= need a teacher")
            object.__setattr__(self, "_distill", None)
            return
        if threshold is not None or guidance_rescale is not None:
            raise ValueError("a thresholded or rescaled teacher is not built: the teacher's two steps use the static clamp")
        if not isinstance(teacher, ViewFusion) or teacher is self:
            raise ValueError("the teacher must be another ViewFusion model")
        if self._self_cond_p is not None or teacher._self_cond_p is not None:
            raise ValueError("distillation on or with a self-conditioned model is not built (DESIGN 8): "
                             "set_self_cond(None) on the student and the teacher first")
        if self._lv_weight is not None or teacher._lv_weight is not None:
            raise ValueError("distillation on or with a learned-variance model is not built (DESIGN 8): "
                             "set_learned_variance(None) on the student and the teacher first")
        if getattr(self, "betas64", None) is None or getattr(teacher, "betas64", None) is None:
            raise ValueError("set_distill needs the noise schedule of both models: call set_new_noise_schedule first")
        import numpy as np
        if teacher.num_timesteps != self.num_timesteps or not np.array_equal(teacher.betas64, self.betas64):
            raise ValueError("the teacher must have the student's noise schedule (the same betas, the same T)")
        if self._in_channels(teacher.denoise_fn) != self._in_channels(self.denoise_fn):
            raise ValueError("the teacher must take the student's input: the same image channels and `relative` "
                             f"configuration ({self._in_channels(teacher.denoise_fn)} input channels against "
                             f"{self._in_channels(self.denoise_fn)})")
        if isinstance(steps, bool) or not isinstance(steps, int):
            raise ValueError(f"steps must be an integer, got {steps!r}")
        tabs = _schedule.distill_tables(self.betas64, steps, teacher.prediction)      # ValueError for K < 1, 2K > T
        if guidance is not None and not torch.is_tensor(guidance) and not isinstance(guidance, (list, tuple)):
            import math
            guidance = float(guidance)
            if not math.isfinite(guidance) or guidance < 0:
                raise ValueError(f"a guidance scale must be finite and >= 0, got {guidance}")
        if self._level_spec is not None:
            raise ValueError("distillation with a level sampler is not built: the student step is drawn uniformly "
                             "(set_level_sampler(None) first)")
        if self._cond_drop_p > 0:
            raise ValueError("distillation with conditioning dropout is not built: a distilled student is not "
                             "w-conditioned (set_cond_dropout(0) first)")
        dev = self.gammas.device
        if teacher.gammas.device != dev:
            raise ValueError(f"the teacher must live on the student's device ({teacher.gammas.device} against {dev})")
        teacher.eval()
        f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)              # noqa: E731
        plan = {k: f32(v) for k, v in tabs["teacher"].items()}
        tau_t = torch.tensor(tabs["tau_t"], dtype=torch.int64, device=dev)
        object.__setattr__(self, "_distill", dict(
            teacher=teacher, steps=int(steps), guidance=guidance, prediction=teacher.prediction, plan=plan,
            level_t=self.gammas[tau_t].contiguous(), tau_s=torch.tensor(tabs["tau_s"], dtype=torch.int64, device=dev),
            w1=f32(tabs["w1"]), w2=f32(tabs["w2"])))

    @staticmethod
    def _in_channels(net):
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                return m.in_channels
        return None

    @torch.no_grad()
    def distill_targets(self, y_cond, view_count, angle, y_0, noise=None, t=None, seed=None, sample_ids=None):
        """The teacher phase of a distillation step (steps 1 - 5 of the definition in csrc/diffusion.hip), under no_grad:
        -> dict(distill_z = z_t, distill_level = gammas[tau_S[i]] (B,), distill_eps = eps~, distill_x0 = x~), the four
        inputs forward() takes in place of running the phase itself (a Trainer runs it in front of its captured step).
        Launches: [noise draw] begin, stack (conditioning half once), the teacher UNet, sampler_step (history buffer),
        level gather + re-stack of the target half, the teacher UNet, distill_target.  Sets `last_distill` = (i, x~)."""
        from . import ops
        d = self._distill
        if d is None:
            raise ValueError("distill_targets needs set_distill(teacher, steps=K)")
        teacher = d["teacher"]
        if teacher.prediction != d["prediction"]:
            raise ValueError("the teacher's prediction changed since set_distill: call set_distill again")
        if self._level_spec is not None or self._cond_drop_p > 0:
            raise ValueError("distillation with a level sampler or conditioning dropout is not built (DESIGN 8)")
        if self.gammas.device.type != "cuda" or teacher.gammas.device != self.gammas.device:
            raise ValueError("distillation runs on the GPU only (its target is formed by HIP kernels), with the teacher "
                             "on the student's device: move both models there and call set_distill again")
        if teacher.training:
            teacher.eval()
        b, dev = y_0.shape[0], y_0.device
        y_0 = y_0.contiguous()
        ids = None
        if seed is not None and (t is None or noise is None):
            ids = ops.sample_ids(dev, b, sample_ids)
        if seed is not None and noise is None:
            noise = ops.randn_ids(seed, ids, ops.diffusion.RNG_TRAIN_NOISE, 0, tuple(y_0.shape[1:]))
        if t is None and seed is None:            # the reference's draw order: the step where t is drawn, then the noise
            t = torch.randint(0, d["steps"], (b,), device=dev)
        if noise is None:
            noise = torch.randn_like(y_0)
        if t is None:
            i, k1, k0, level, z_t = ops.distill_begin(y_0, noise, d["tau_s"], self.gammas, seed=seed, ids=ids)
        else:
            i, k1, k0, level, z_t = ops.distill_begin(y_0, noise, d["tau_s"], self.gammas, i=t.to(torch.int64))
        gs = None if d["guidance"] is None else ops.guidance_scales(dev, b, d["guidance"])
        guided = gs is not None
        off, S, max_v = ops.view_offsets(view_count, dev)
        w_on = bool(teacher.weighting_inference)
        y_cond, angle = y_cond.contiguous(), angle.contiguous()
        y, x1 = z_t.clone(), torch.empty_like(z_t)                 # the teacher's chain moves y in place; x1: its history
        x, out = teacher._denoise(y, y_cond, angle, k1, off, S, levels=d["level_t"], null_rows=guided)
        ops.sampler_step(out, off, y, None, k1, d["plan"], b, max_v, w_on, y0_prev=x1, want_weights=False, inplace=True,
                         guidance=gs, S=S)
        _, out = teacher._denoise(y, y_cond, angle, k0, off, S, x=x, copy_cond=False, levels=d["level_t"],
                                  null_rows=guided)
        x_t, eps_t = ops.distill_target(out, off, y, x1, z_t, level, i, k0, d["plan"], d["w1"], d["w2"], b, w_on,
                                        guidance=gs, S=S)
        self.last_distill = (i, x_t)
        return dict(distill_z=z_t, distill_level=level, distill_eps=eps_t, distill_x0=x_t)

    # -- self-conditioning --------------------------------------------------------------------
    def set_self_cond(self, p=0.5):
        """Self-conditioning (Chen et al., "Analog Bits", 2.2; csrc/diffusion.hip holds the definition).
        set_self_cond(None), the default: off -- every launch and every bit as before.

        The network -- UNet(in_channel = Cc + 6), Cc the conditioning views' channels -- is also shown an estimate of the
        clean image, as three more input channels behind the noisy target; zeros mean "no estimate".
        Training: forward() first runs the network once under no_grad, without Dropout and with zeros there, turns its
        composed output into x^ = clamp(a y_t - b out, -1, 1) and keeps it per sample with probability p (seeded: word 3
        of the call that gives the sample's t and u, ops.draw_self_cond; unseeded: torch.rand(B) < p after every other
        draw); the ordinary step then sees x^ and takes the ordinary objective.  No gradient flows through the first
        pass.  p = 0 runs no first pass; in eval mode every sample keeps its estimate and nothing is drawn.
        forward(self_cond=x) injects the (already masked) estimate instead; self_cond_targets() is the first pass on its
        own; `last_self_cond` = (keep uint8 (B,), x^) of the last one.
        Sampling: generate() feeds back the y0 the previous step's tail wrote (zeros at the first step); p_sample /
        p_mean_variance take self_cond= (None: zeros).
        A plain attribute (`self_cond` reads it back): no buffer, no parameter -- save it as
        save_checkpoint(..., self_cond=model.self_cond).  A Trainer drops its captured steps when it changes and runs the
        first pass in front of every (micro-)step.  Refused with ValueError: together with set_distill (on
        either model) or a level sampler and, when it runs, a CPU model or a network whose input is not Cc + 6 channels."""
        if p is None:
            self._self_cond_p = None
            self.last_self_cond = None
            return
        p = float(p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"the self-conditioning probability must be in [0, 1], got {p}")
        if self._distill is not None:
            raise ValueError("self-conditioning on a distillation student is not built (DESIGN 8): set_distill(None) first")
        if self._level_spec is not None:
            raise ValueError("self-conditioning together with a level sampler is not built (DESIGN 8): "
                             "set_level_sampler(None) first")
        if self._lv_weight is not None:
            raise ValueError("self-conditioning together with a learned variance is not built (DESIGN 8): "
                             "set_learned_variance(None) first")
        self._self_cond_p = p

    @property
    def self_cond(self):
        """The self-conditioning probability p of set_self_cond, None while it is off."""
        return self._self_cond_p

    def _check_self_cond(self, Cc, dev):
        """ValueError, before any launch, where a self-conditioned pass cannot run: a CPU model, or a network whose stem
        does not take [ cond (Cc) | noisy target (3) | estimate (3) ]."""
        have = self._in_channels(self.denoise_fn)
        if have is not None and have != Cc + 6:
            raise ValueError(f"a self-conditioned model stacks {Cc} conditioning + 3 target + 3 estimate channels = "
                             f"{Cc + 6}, the network takes in_channel = {have}")
        if torch.device(dev).type != "cuda":
            raise ValueError("self-conditioning runs on the GPU only (its stacking and its estimate are HIP kernels): move "
                             "the model and the batch there")

    def _history_buffer(self, y):
        """The buffer the few-step tail writes the step's y0 into (dpmpp2m's history; a self-conditioned chain's estimate)."""
        return torch.empty_like(y)

    @torch.no_grad()
    def self_cond_targets(self, y_cond, view_count, angle, y_0, noise=None, t=None, u=None, cond_drop=None, seed=None,
                          sample_ids=None):
        """The first pass of a self-conditioned training step (csrc/diffusion.hip), under no_grad: draws whatever is not
        injected exactly as forward() would -- same order, same kernels -- then the coin, stacks the input with zero
        estimate channels, runs the network on its inference path (no Dropout) and forms the masked estimate x^.
        -> the dict forward() takes in place of running the phase itself: always `self_cond`; without seed= also the `t`,
        `u`, `noise` (and `cond_drop`) it used, so that the step that follows uses the same ones (with seed= that step
        draws them again from the same counters).  p = 0: no pass, `self_cond` is None (forward stacks zeros).
        Sets `last_self_cond` = (keep uint8 (B,), x^)."""
        from . import ops
        from .unet import UNet
        p = self._self_cond_p
        if p is None:
            raise ValueError("self_cond_targets needs set_self_cond(p)")
        if self._distill is not None or self._level_spec is not None:
            raise ValueError("self-conditioning with distillation or a level sampler is not built (DESIGN 8)")
        b, dev = y_0.shape[0], y_0.device
        self._check_self_cond(y_cond.shape[2], dev)
        # forward()'s draws, in forward()'s order
        drop_p = self._cond_drop_p if (cond_drop is None and self.training) else 0.0
        drop, level, ids = cond_drop, None, sample_ids
        if seed is not None:
            ids = ops.sample_ids(dev, b, sample_ids)
            if drop_p > 0:
                drop = ops.draw_cond_drop(seed, ids, drop_p)
            if t is None or u is None:
                t_d, level_d, u_d = ops.draw_train(seed, ids, self.gammas, want_u=t is not None)
                if t is None and u is None:
                    t, level = t_d, level_d
                elif t is None:
                    t = t_d
                else:
                    u = u_d
            if noise is None:
                noise = ops.randn_ids(seed, ids, ops.diffusion.RNG_TRAIN_NOISE, 0, tuple(y_0.shape[1:]))
        if t is None:
            t = torch.randint(1, self.num_timesteps, (b,), device=dev).long()
        if u is None and level is None:
            u = torch.rand((b, 1), device=dev)
        if noise is None:
            noise = torch.randn_like(y_0)
        if drop is None and drop_p > 0:
            drop = torch.rand(b, device=dev) < drop_p
        res = {} if seed is not None else dict(t=t, u=u, noise=noise)
        if seed is None and drop is not None:
            res["cond_drop"] = drop
        # the coin: after every other draw; eval mode keeps every sample and draws nothing
        if not self.training:
            keep = None
        elif seed is not None:
            keep = ops.draw_self_cond(seed, ids, p) if p > 0 else None
        else:
            keep = (torch.rand(b, device=dev) < p).view(torch.uint8) if p > 0 else None
        if self.training and p == 0:
            self.last_self_cond = (torch.zeros(b, dtype=torch.uint8, device=dev), None)
            res["self_cond"] = None
            return res
        if level is None:
            level = ops.gather_level(self.gammas, t, u.reshape(-1).contiguous())
        off, S, _ = ops.view_offsets(view_count, dev)
        x, level_s, angle_s = ops.stack_views(y_cond, y_0.contiguous(), noise.contiguous(), level, angle, off, S,
                                              drop=drop, sc_channels=True)
        fn = self.denoise_fn
        out = fn(x, angle_s, level_s, **({"no_dropout": True} if isinstance(fn, UNet) else {}))
        x_hat = ops.self_cond_estimate(out, off, level, b, bool(self.weighting_train), self.prediction, x=x, keep=keep)
        self.last_self_cond = (torch.ones(b, dtype=torch.uint8, device=dev) if keep is None else keep, x_hat)
        res["self_cond"] = x_hat
        return res

    def loss_key(self):
        """What a captured training step depends on besides its inputs: the objective, the attached histogram, the
        conditioning-dropout probability, the level sampler (every set_level_sampler call counts), the prediction, the
        distillation settings (every set_distill call counts), the self-conditioning probability and the vlb weight of a
        learned variance."""
        h = self.loss_hist
        return (None if self._loss is None else tuple(sorted(self._loss.items(), key=lambda kv: kv[0])),
                None if h is None else (h[0].data_ptr(), h[1].data_ptr(), h[0].numel()), self._cond_drop_p,
                self._level_gen, self.prediction, self._distill_gen, self._self_cond_p, self._lv_weight)

    # -- schedule ---------------------------------------------------------------------------
    def set_new_noise_schedule(self, device=torch.device("cuda"), phase="train"):
        betas = _schedule.make_beta_schedule(**self.beta_schedule[phase])
        self.num_timesteps = int(betas.shape[0])
        self.betas64 = betas                   # float64, for the few-step sampler tables; not a buffer (state_dict)
        self._plan = None
        self._pred_tabs = None
        self._lv_tabs = None
        self._nll_plan = None                  # the tables of a bound evaluation (bound_terms), made on demand
        self._eps_plan = None                  # the tables of a moment estimation (eps_moments), made on demand
        for name, val in _schedule.schedule_tensors(betas, device).items():
            if name in self._buffers:
                self._buffers[name] = val
            else:
                self.register_buffer(name, val)

    def _sched(self):
        """The tables the ancestral tail reads.  "eps": the very buffers.  "v" / "x0": the same posterior buffers, and the
        prediction's (a, b) pair under the two names the tail reads y0_hat's coefficients from."""
        sched = {k: getattr(self, k) for k in _schedule.BUFFER_NAMES}
        if self.prediction == "eps":
            return sched
        dev = self.gammas.device
        if self._pred_tabs is None or self._pred_tabs[0] != (self.prediction, dev):
            a, b = _schedule.prediction_tables(self.betas64, self.prediction)
            self._pred_tabs = ((self.prediction, dev), torch.tensor(a, dtype=torch.float32, device=dev),
                               torch.tensor(b, dtype=torch.float32, device=dev))
        sched["sqrt_recip_gammas"], sched["sqrt_recipm1_gammas"] = self._pred_tabs[1], self._pred_tabs[2]
        return sched

    def _check_samplable(self):
        """ValueError, before any launch, where y0_hat cannot be formed: "eps" at a level with gamma = 0."""
        if self.prediction == "eps" and float(self.betas64[-1]) >= 1.0:
            raise ValueError("an eps-prediction model cannot sample on a zero-terminal-SNR schedule (gamma_T = 0: g^-1/2 "
                             "is infinite there); use set_prediction('v') or 'x0'")

    def _sampler_plan(self, tau, solver, eta, device, variance=None):
        """The device side of a few-step chain: the fp32 tables of schedule.sampler_tables, `tau` as int64 and
        `level` = the fp32 `gammas` buffer gathered at tau (the network sees the very levels of the full chain).
        `noisy[k]`: sigma[k] != 0, on the host.  The last plan is kept (evaluate() asks for the same one per batch).
        variance="analytic": the sigma row is the analytic one of the model's moments (set_moments), and `noisy` follows
        it; the moments are part of the key."""
        key = (tuple(int(v) for v in tau), solver, float(eta), device, self.prediction,
               None if variance is None else (variance, self._moments_gen))
        if self._plan is None or self._plan[0] != key:
            tab = _schedule.sampler_tables(self.betas64, tau, solver, eta, self.prediction,
                                           **({} if variance is None else dict(moments=self._moments)))
            host = {k: torch.tensor(v, dtype=torch.float32) for k, v in tab.items()}
            plan = {k: v.to(device) for k, v in host.items()}
            plan["tau"] = torch.tensor(tau, dtype=torch.int64, device=device)
            plan["level"] = self.gammas[plan["tau"]].contiguous()
            plan["noisy"] = (host["sigma"] != 0).tolist()
            plan["multistep"] = bool((host["c1"] != 0).any())
            self._plan = (key, plan)
        return self._plan[1]

    @staticmethod
    def _at(table, t, ndim=4):
        return table.gather(-1, t).reshape(t.shape[0], *((1,) * (ndim - 1)))

    # -- small API-compat helpers (not on the fused hot path) ---------------------------------
    def predict_start_from_noise(self, y_t, t, noise):
        return self._at(self.sqrt_recip_gammas, t) * y_t - self._at(self.sqrt_recipm1_gammas, t) * noise

    def predict_start(self, y_t, t, out):
        """y0_hat = a[t] y_t - b[t] out for the model's own prediction (predict_start_from_noise under "eps")."""
        sched = self._sched()
        return self._at(sched["sqrt_recip_gammas"], t) * y_t - self._at(sched["sqrt_recipm1_gammas"], t) * out

    def q_posterior(self, y_0_hat, y_t, t):
        mean = self._at(self.posterior_mean_coef1, t) * y_0_hat + self._at(self.posterior_mean_coef2, t) * y_t
        return mean, self._at(self.posterior_log_variance_clipped, t)

    def q_sample(self, y_0, sample_gammas, noise=None):
        if noise is None:
            noise = torch.randn_like(y_0)
        return sample_gammas.sqrt() * y_0 + (1 - sample_gammas).sqrt() * noise

    # -- reverse process ---------------------------------------------------------------------
    def _denoise(self, y_t, y_cond, angle, t, off, S, x=None, copy_cond=True, levels=None, null_rows=False, sc=None):
        """sc (default None: the launches of before): the self-conditioning keywords of ops.stack_views."""
        from . import ops
        level = ops.gather_level(self.gammas if levels is None else levels, t)
        x, level_s, angle_s = ops.stack_views(y_cond, y_t, None, level, angle, off, S, x=x, copy_cond=copy_cond,
                                              null_rows=null_rows, **(sc or {}))
        return x, self.denoise_fn(x, angle_s, level_s)

    def _sc_step(self, y_t, y_cond, self_cond):
        """The stack_views keywords of one self-conditioned reverse step (None while the feature is off and no estimate
        is handed over): checked before any launch."""
        if self_cond is None and self._self_cond_p is None:
            return None
        self._check_self_cond(y_cond.shape[2], y_t.device)
        if self_cond is not None and tuple(self_cond.shape) != tuple(y_t.shape):
            raise ValueError(f"self_cond must have y_t's shape {tuple(y_t.shape)}, got {tuple(self_cond.shape)}")
        return dict(self_cond=None if self_cond is None else self_cond.contiguous(), sc_channels=True)

    def p_mean_variance(self, y_t, y_cond, view_count, angle, t, clip_denoised: bool, guidance=None, threshold=None,
                        threshold_max=None, guidance_rescale=None, self_cond=None):
        """guidance (a scale, or one per sample): the mean of the guided step; logits are the S conditional rows'.
        threshold / threshold_max / guidance_rescale: as in generate().
        self_cond (B,3,H,W; a self-conditioned model, set_self_cond): the estimate shown to the network; None is zeros."""
        from . import ops
        ops.threshold_settings(threshold, threshold_max, guidance_rescale, guidance is not None, clip_denoised)
        self._check_samplable()
        if self._lv_weight is not None:
            self._check_lv(y_t.device, threshold, guidance_rescale)
            if not clip_denoised:
                raise ValueError("the learned-variance step clamps y0_hat: clip_denoised=False is not built")
        sc = self._sc_step(y_t, y_cond, self_cond)
        dyn = dict(threshold=threshold, threshold_max=threshold_max, guidance_rescale=guidance_rescale)
        gs = None if guidance is None else ops.guidance_scales(y_t.device, y_t.shape[0], guidance)
        off, S, max_v = ops.view_offsets(view_count, y_t.device)
        _, out = self._denoise(y_t, y_cond, angle, t, off, S, null_rows=gs is not None, sc=sc)
        w_on = bool(self.weighting_inference)
        if self._lv_weight is not None:   # the learned step without noise is the mean; its log-variance is per pixel
            plan = self._lv_plan(list(range(self.num_timesteps)), y_t.device)
            mean, weights, lp = ops.sampler_step(out, off, y_t, None, t, plan, y_t.shape[0], max_v, w_on, guidance=gs, S=S,
                                                 variance=(plan["hi"], plan["lo"]), want_logvar=True)
            return mean, lp, (self._logits(out, S) if w_on else None), weights
        _, mean, weights = ops.p_sample_tail(out, off, y_t, None, t, self._sched(), y_t.shape[0], max_v, w_on,
                                             clip=clip_denoised, want_mean=True, guidance=gs, S=S, **dyn)
        logits = out[:S, 3:, ...] if w_on else None
        return mean, self._at(self.posterior_log_variance_clipped, t), logits, weights

    @torch.no_grad()
    def p_sample(self, y_t, y_cond, view_count, angle, t, clip_denoised=True, z=None, guidance=None, threshold=None,
                 threshold_max=None, guidance_rescale=None, self_cond=None, variance=None):
        """self_cond (B,3,H,W; a self-conditioned model): the estimate shown to the network; None is zeros.
        variance="analytic" (default None: the step as before): the ancestral step with the analytic noise scale of the
        model's moments in place of the posterior one -- step t of generate(variance="analytic") on the full chain, through
        the table-driven tail, which clamps y0_hat (clip_denoised=False is refused)."""
        from . import ops
        ops.threshold_settings(threshold, threshold_max, guidance_rescale, guidance is not None, clip_denoised)
        self._check_samplable()
        if variance is not None:
            if variance != _schedule.ANALYTIC_VARIANCE:
                raise ValueError(f"unknown variance {variance!r}: None or {_schedule.ANALYTIC_VARIANCE!r}")
            self._check_analytic(y_t.device, "variance='analytic'")
            if not clip_denoised:
                raise ValueError("the table-driven step clamps y0_hat: clip_denoised=False is not built")
        if self._lv_weight is not None:
            self._check_lv(y_t.device, threshold, guidance_rescale)
            if not clip_denoised:
                raise ValueError("the learned-variance step clamps y0_hat: clip_denoised=False is not built")
        sc = self._sc_step(y_t, y_cond, self_cond)
        dyn = dict(threshold=threshold, threshold_max=threshold_max, guidance_rescale=guidance_rescale)
        gs = None if guidance is None else ops.guidance_scales(y_t.device, y_t.shape[0], guidance)
        off, S, max_v = ops.view_offsets(view_count, y_t.device)
        _, out = self._denoise(y_t, y_cond, angle, t, off, S, null_rows=gs is not None, sc=sc)
        if z is None:
            z = torch.randn_like(y_t) if bool((t > 0).any()) else None
        elif not bool((t > 0).any()):
            z = None
        w_on = bool(self.weighting_inference)
        if self._lv_weight is not None:   # sigma[0] == 0: the tail reads no z at t = 0 (one t for the batch, as generate)
            plan = self._lv_plan(list(range(self.num_timesteps)), y_t.device)
            y, weights = ops.sampler_step(out, off, y_t, z, t, plan, y_t.shape[0], max_v, w_on, guidance=gs, S=S,
                                          variance=(plan["hi"], plan["lo"]))
            return y, (self._logits(out, S) if w_on else None), weights
        if variance is not None:          # the "ddim", eta = 1 tables of the full chain with the analytic sigma row
            plan = self._sampler_plan(list(range(self.num_timesteps)), "ddim", 1.0, y_t.device, variance)
            y, weights = ops.sampler_step(out, off, y_t, z, t, plan, y_t.shape[0], max_v, w_on, guidance=gs, S=S, **dyn)
            return y, (out[:S, 3:, ...] if w_on else None), weights
        y, _, weights = ops.p_sample_tail(out, off, y_t, z, t, self._sched(), y_t.shape[0], max_v, w_on,
                                          clip=clip_denoised, guidance=gs, S=S, **dyn)
        return y, (out[:S, 3:, ...] if w_on else None), weights

    @torch.no_grad()
    def generate(self, y_cond, view_count, angle, y_t=None, sample_num=8, z_seq=None, use_graph=None, seed=None,
                 sample_ids=None, sample_steps=None, solver="ddim", eta=0.0, guidance=None, threshold=None,
                 threshold_max=None, guidance_rescale=None, variance=None):
        """Reverse diffusion over all T steps (reference view_fusion.py:179-214).

        use_graph (default: on for GPU tensors with S <= 16 stacked views): one reverse step -- level gather, re-stack of
        y_t, the whole UNet forward and the fused compose/posterior tail (~260 launches) -- is
        captured once into a HIP graph and replayed T times, so the loop is not launch-bound at
        small S.  Per step the host only refreshes the step index and the noise buffer.

        seed (default None: torch's device generator): y_T and every step's z come from the counter-based generator
        (csrc/rng.h), keyed by `sample_ids` (default arange(B)); z is computed inside the tail kernel, so the host
        only refreshes the step index.  An injected y_t / z_seq still wins, each on its own.

        sample_steps (default None: the ancestral chain above, untouched): K, or an explicit increasing sequence of
        timesteps ending at T-1 -- a K-step chain over the sub-sequence schedule.sample_timesteps(T, K) of the trained
        levels with solver "ddim" (eta in [0, 1]; 0 deterministic, 1 ancestral) or "dpmpp2m" (DPM-Solver++ 2M, eta 0).
        The loop is the same one, with the table-driven tail (ops.sampler_step) and the step index k in place of t;
        z_seq stays (T, ...) and is read at the model timestep, z_seq[tau[k]]; snapshots where k % (K // sample_num) == 0.

        guidance (default None: everything above, launch for launch): a classifier-free guidance scale g >= 0, or one per
        sample as a (B,) tensor.  The stacked batch gets one null row per sample after the S real ones -- the sample's
        noisy target next to an all-zero conditioning half, its own level and angle -- so the UNet sees S + B rows, and
        every tail (ancestral or few-step, loaded or drawn z) uses eps = g eps_c + (1 - g) eps_u.  g = 1 is the
        unguided sampler, g = 0 the unconditional model, g > 1 extrapolates.  The returned logits are those of the S
        real rows and the weights stay the conditional softmax; the use_graph default compares S + B.

        threshold (default None: the static clamp to [-1, 1]): q in (0, 1] -- dynamic thresholding, every step: s = the
        q-quantile of |y0_hat| over the sample's 3 H W values (torch.quantile's interpolation), at least 1 and at most
        threshold_max (c >= 1) when that is given; y0 = clamp(y0_hat, -s, s) / s.
        guidance_rescale (default None; 0 is "off"; needs guidance): phi in (0, 1] -- the guided noise is multiplied by
        phi sigma(eps_c) / sigma(eps_g) + 1 - phi, per sample, which takes its standard deviation back to (phi = 1) the
        conditional prediction's.  Either one turns the tail into three launches (composed eps, per-sample statistics,
        tail) that stay inside the captured step; their scratch buffers are made once per call.  Both combine with
        everything above.  No schedule of q / phi over the steps.

        A self-conditioned model (set_self_cond; csrc/diffusion.hip): the estimate channels of every step's input are the
        y0 the step before wrote into the few-step tail's history buffer -- clamped or thresholded, guided -- and zeros at
        the first step; with dpmpp2m the tail's own history is that same buffer.  Only the table-driven tail hands y0 back,
        so sample_steps=None runs as sample_steps=T, solver="ddim", eta=1.0: the ancestral chain through that tail (the
        sampler tests pin the two to each other within the chain tolerance).  Everything above combines with it unchanged.

        variance (default None: everything above, launch for launch and bit for bit): "analytic" -- the Analytic-DPM
        optimal variance (Bao et al.; csrc/diffusion.hip holds the definition).  The table-driven chain with
        solver="ddim" at the given eta, its mean unchanged and its sigma row replaced by the KL-optimal one of the
        model's moments (set_moments; schedule.analytic_sigma2), sigma*[0] = 0: the same launches as that chain, only a
        table row differs.  eta = 0 is Analytic-DDIM, which is STOCHASTIC (sigma*^2 = c0^2 (1 - g)/g (1 - M) > 0): it
        draws z where "ddim", eta = 0 draws none.  sample_steps=None runs as sample_steps=T, solver="ddim", eta=1.0.
        The moments are those of the unguided model without thresholding: guidance / threshold / guidance_rescale run
        (only a table row differs) but nothing is claimed for them.  ValueError before any launch: solver="dpmpp2m", no
        moments set, a learned-variance model, a CPU model.
        """
        from . import ops
        q_on, _, phi = ops.threshold_settings(threshold, threshold_max, guidance_rescale, guidance is not None)
        dyn = {}
        plan = tau = None
        self._check_samplable()
        if variance is not None:                          # only the table-driven tail reads a sigma row
            if variance != _schedule.ANALYTIC_VARIANCE:
                raise ValueError(f"unknown variance {variance!r}: None or {_schedule.ANALYTIC_VARIANCE!r}")
            if sample_steps is not None and solver != "ddim":
                raise ValueError("variance='analytic' goes with solver='ddim' alone: dpmpp2m is deterministic (DESIGN 8)")
            self._check_analytic(y_cond.device, "variance='analytic'")
            if sample_steps is None:
                sample_steps, solver, eta = self.num_timesteps, "ddim", 1.0
        lv_on = self._lv_weight is not None
        if lv_on:                                         # only the table-driven tail has the learned-variance flavour
            self._check_lv(y_cond.device, threshold, guidance_rescale)
            if sample_steps is None:
                sample_steps, solver, eta = self.num_timesteps, "ddim", 1.0
        sc_on = self._self_cond_p is not None
        if sc_on:                                         # only the table-driven tail hands y0 back
            self._check_self_cond(y_cond.shape[2], y_cond.device)
            if sample_steps is None:
                sample_steps, solver, eta = self.num_timesteps, "ddim", 1.0
        if sample_steps is not None:                      # argument errors first: nothing has been launched yet
            _schedule.check_sampler(solver, eta)
            tau = _schedule.sample_timesteps(self.num_timesteps, sample_steps).tolist()
            if variance is not None:                      # a level with gamma = 0 or without a moment: refused here
                _schedule.analytic_sampler_sigma(self.betas64, tau, self._moments, eta)
        b = y_cond.shape[0]
        gs = None if guidance is None else ops.guidance_scales(y_cond.device, b, guidance)
        guided = gs is not None
        assert self.num_timesteps > sample_num, "num_timesteps must greater than sample_num"
        n_steps = self.num_timesteps if tau is None else len(tau)
        every = max(1, n_steps // sample_num)
        ids = None if seed is None else ops.sample_ids(y_cond.device, b, sample_ids)
        if y_t is None and seed is not None:
            y_t = ops.randn_ids(seed, ids, ops.diffusion.RNG_START_NOISE, 0, (3,) + tuple(y_cond.shape[-2:]))
        elif y_t is None:
            y_t = torch.randn_like(y_cond[:, :1, :3, ...]).squeeze(dim=1)
        y = y_t.contiguous().clone()                      # updated in place, step after step
        dev = y.device
        off, S, max_v = ops.view_offsets(view_count, dev)
        w_on = bool(self.weighting_inference)
        sched = self._sched()
        if use_graph is None:                             # measured: replay wins while the step is launch-bound
            use_graph = y.is_cuda and S + (b if guided else 0) <= 16   # (at S = 12 replay and eager tie, but replay is immune to host jitter)
        t = torch.full((b,), n_steps - 1, device=dev, dtype=torch.long)     # the step index: t, or k of a few-step chain
        z_seed = seed if z_seq is None else None          # the tail draws z itself: no noise buffer
        z = None if z_seed is not None else torch.zeros_like(y)
        levels, hist = self.gammas, None
        if tau is not None:
            lv_step = lv_on and solver == "ddim" and float(eta) == 1.0
            plan = self._lv_plan(tau, dev) if lv_step else self._sampler_plan(tau, solver, eta, dev, variance)
            lv = dict(variance=(plan["hi"], plan["lo"])) if lv_step else {}
            levels = plan["level"]
            # y0 of the step before; the multistep tail never reads it first ...
            hist = self._history_buffer(y) if plan["multistep"] or sc_on else None
            if sc_on:                                     # ... but the stacking reads it at the top of EVERY step: zeros
                hist.zero_()                              # = "no estimate" before the first one
            if not any(plan["noisy"]):                    # eta = 0: no z anywhere -- no buffer, no draw
                z_seed = z = None
        if q_on is not None or phi > 0.0:                 # the three-launch tail and what it keeps between its launches
            dyn = dict(threshold=threshold, threshold_max=threshold_max, guidance_rescale=guidance_rescale,
                       scratch=ops.threshold_scratch(y))
        y_cond = y_cond.contiguous()
        angle = angle.contiguous()
        # the conditioning half of the stacked input never changes: copy it once (guided: the null rows' zeros too)
        # (self-conditioned: the sibling kernel, whose third part is the history buffer the tail below writes)
        sc = dict(self_cond=hist, sc_channels=True) if sc_on else {}
        x, _, _ = ops.stack_views(y_cond, y, None, ops.gather_level(levels, t), angle, off, S, null_rows=guided, **sc)

        def step():
            _, out = self._denoise(y, y_cond, angle, t, off, S, x=x, copy_cond=False, levels=levels, null_rows=guided,
                                   sc=sc)
            if plan is not None:
                _, weights = ops.sampler_step(out, off, y, z, t, plan, b, max_v, w_on, y0_prev=hist, inplace=True,
                                              seed=z_seed, ids=ids, guidance=gs, S=S, **dyn, **lv)
                return out, weights
            _, _, weights = ops.p_sample_tail(out, off, y, z, t, sched, b, max_v, w_on, inplace=True, seed=z_seed,
                                              ids=ids, guidance=gs, S=S, **dyn)
            return out, weights

        graph = None
        if use_graph:
            y0 = y.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                 # warm-up: packs weights, fills caches
                step()
            torch.cuda.current_stream().wait_stream(side)
            y.copy_(y0)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out, weights = step()
            y.copy_(y0)                                    # capture does not execute, but be explicit
            if sc_on:                                      # the warm-up step wrote its y0 into the history buffer
                hist.zero_()

        ret, logit_arr, weight_arr = [y_t], [], []
        for i in reversed(range(n_steps)):
            t.fill_(i)
            if z is None:                                  # seeded: the tail kernel draws z (0 at step 0) itself
                pass
            elif (i == 0) if plan is None else (not plan["noisy"][i]):
                z.zero_()
            elif z_seq is not None:
                z.copy_(z_seq[i if tau is None else tau[i]])          # z_seq is indexed by the model timestep
            else:
                z.normal_()
            if graph is not None:
                graph.replay()
            else:
                out, weights = step()
            if i % every == 0:
                ret.append(y.clone())
                logit_arr.append(self._logits(out, S).clone() if w_on else None)
                weight_arr.append(weights.clone() if w_on else None)
        ret = torch.stack(ret, dim=1)
        samples = ret[:, -1, ...]
        if w_on:
            logit_arr = torch.stack(logit_arr, dim=1)
            weight_arr = torch.stack(weight_arr, dim=1)
        return y, ret, logit_arr, weight_arr, samples

    sample = generate

    # -- the variational bound -----------------------------------------------------------------
    def _nll_plan_for(self, tau, fixed_variance, dev):
        """The device side of a bound evaluation: the fp32 tables of schedule.nll_tables, `tau` as int64, `level` = the
        fp32 `gammas` buffer gathered at tau and `snr` = level / (1 - level) (formed in float64, rounded once).  The
        last plan is kept (bits_per_dim asks for the same one per batch)."""
        analytic = fixed_variance == _schedule.ANALYTIC_VARIANCE
        key = (tuple(int(v) for v in tau), self.prediction, fixed_variance, dev, self._moments_gen if analytic else None)
        plan = getattr(self, "_nll_plan", None)
        if plan is None or plan[0] != key:
            tab = _schedule.nll_tables(self.betas64, tau, self.prediction, fixed_variance,
                                       **(dict(moments=self._moments) if analytic else {}))
            new = {k: torch.tensor(v, dtype=torch.float32, device=dev) for k, v in tab.items()}
            new["tau"] = torch.tensor(list(key[0]), dtype=torch.int64, device=dev)
            new["level"] = self.gammas[new["tau"]].contiguous()
            g = new["level"].double()
            new["snr"] = (g / (1.0 - g)).float()
            plan = self._nll_plan = (key, new)
        return plan[1]

    def _check_bound(self, dev, fixed_variance="small", guidance=None, threshold=None, guidance_rescale=None):
        """ValueError, before any launch, where the bound cannot be evaluated (bound_terms; drivers.evaluate(nll=True)
        asks before its first generate()): `dev` is where the targets live."""
        if guidance is not None or threshold is not None or \
                (guidance_rescale is not None and float(guidance_rescale) > 0):
            raise ValueError("bound_terms takes no guidance / threshold / guidance_rescale: the bound is that of the "
                             "conditional model's own reverse process (DESIGN 8)")
        if self._self_cond_p is not None:
            raise ValueError("the bound of a self-conditioned model is not built (DESIGN 8): its reverse step depends on "
                             "the chain's own history")
        if fixed_variance not in _schedule.BOUND_VARIANCES:
            raise ValueError(f"unknown fixed_variance {fixed_variance!r}: one of {_schedule.BOUND_VARIANCES}")
        if fixed_variance == _schedule.ANALYTIC_VARIANCE:
            self._check_analytic(dev, "fixed_variance='analytic'")
        if self._lv_weight is not None and fixed_variance == "large":
            raise ValueError("fixed_variance='large' on a model with a learned variance: the model has its own")
        if torch.device(dev).type != "cuda" or self.gammas.device.type != "cuda":
            raise ValueError("bound_terms runs on the GPU only (its terms are HIP kernels): move the model and the batch "
                             "there")
        if self._lv_weight is not None:
            self._check_lv(dev)

    @torch.no_grad()
    def bound_terms(self, y_cond, view_count, angle, y_0, noise=None, seed=None, sample_ids=None, sample_steps=None,
                    clip_denoised=True, fixed_variance="small", guidance=None, threshold=None, guidance_rescale=None):
        """The variational bound on -log2 p(y_0) of held-out targets, term by term, in bits per dimension (Improved
        DDPM's calc_bpd_loop on this engine; csrc/diffusion.hip holds the definition).  For every step k of the chain
        -- 0..T-1, or sample_steps (K, or an explicit sequence: schedule.sample_timesteps) -- one noisy target y_k per
        sample, one no-grad forward on the inference path at the level gammas[tau[k]] (no Dropout, whatever mode the model
        is in) and one term: the KL of the true posterior from the model's reverse step for k >= 1, the discretised decoder
        likelihood at k = 0; plus the prior term.  The model's variance: learned (set_learned_variance on a nine-channel
        network), else fixed_variance "small" (the posterior variance, what the ancestral sampler uses), "large" (beta) or
        "analytic" (the Analytic-DPM optimal variance of the model's moments, set_moments: the term kernel runs as for
        "large" on another hi row, schedule.nll_tables; refused on a learned variance and without moments).
        noise (B, K, 3, H, W) wins; else seed= draws it from the counter-based generator (kind 6, keyed by sample_ids and
        the model timestep, so a sample's targets do not depend on its batch); else torch's device generator.
        Returns {"total_bpd" (B,), "prior_bpd" (B,), "vb" (B, K), "x0_mse" (B, K), "eps_mse" (B, K), "tau" (K,)}: device
        tensors, no host sync inside the loop; x0_mse is the mean of (y0 - y_0)^2 and eps_mse = x0_mse g / (1 - g).
        Launched eagerly, launch by launch (a captured step is not built).  Refused with ValueError before any launch:
        guidance / threshold / guidance_rescale (a guided model's "bound" is no bound), a self-conditioned model,
        fixed_variance="large" on a learned variance, a CPU model.  A nine-channel network with the learned variance off
        is evaluated as a fixed variance; channels 6..8 are ignored, as the samplers do."""
        from . import ops
        dev = y_0.device
        self._check_bound(dev, fixed_variance, guidance, threshold, guidance_rescale)
        lv = self._lv_weight is not None
        b, _, H, W = y_0.shape
        T = self.num_timesteps
        tau = list(range(T)) if sample_steps is None else _schedule.sample_timesteps(T, sample_steps).tolist()
        K = len(tau)
        if noise is not None and tuple(noise.shape) != (b, K, 3, H, W):
            raise ValueError(f"noise must have shape {(b, K, 3, H, W)}, got {tuple(noise.shape)}")
        if tuple(y_cond.shape[-2:]) != (H, W) or y_cond.shape[0] != b:
            raise ValueError(f"y_cond {tuple(y_cond.shape)} does not go with y_0 {tuple(y_0.shape)}")
        plan = self._nll_plan_for(tau, fixed_variance, dev)      # (ValueError: "eps" at a level with gamma = 0)
        ids = None if seed is None or noise is not None else ops.sample_ids(dev, b, sample_ids)
        off, S, _ = ops.view_offsets(view_count, dev)
        y_0, y_cond, angle = y_0.contiguous(), y_cond.contiguous(), angle.contiguous()
        w_on = bool(self.weighting_inference)
        kidx = torch.zeros(b, device=dev, dtype=torch.int64)
        vb = torch.zeros(b, K, device=dev, dtype=torch.float32)
        mse = torch.zeros(b, K, device=dev, dtype=torch.float32)
        scratch = ops.nll_scratch(b, dev)
        y_k = torch.empty_like(y_0)
        draw = dict(noise=noise.contiguous()) if noise is not None else dict(seed=seed, ids=ids)
        z = zero = None
        if noise is None and seed is None:                       # torch's device generator: one step's draw at a time
            z = torch.empty(b, 1, 3, H, W, device=dev, dtype=torch.float32)
            zero = torch.zeros(b, device=dev, dtype=torch.int64)
        x = None
        was = self.denoise_fn.training if isinstance(self.denoise_fn, nn.Module) else None
        if was:
            self.denoise_fn.eval()
        try:
            for k in reversed(range(K)):
                kidx.fill_(k)
                if z is not None:
                    ops.nll_noisy(y_0, zero, plan["tau"][k:k + 1], self.gammas, noise=z.normal_(), out=y_k)
                else:
                    ops.nll_noisy(y_0, kidx, plan["tau"], self.gammas, out=y_k, **draw)
                x, out = self._denoise(y_k, y_cond, angle, kidx, off, S, x=x, copy_cond=x is None, levels=plan["level"])
                ops.nll_terms(out, off, y_k, y_0, kidx, plan, b, w_on, learned=lv, decoder=k == 0,
                              large=fixed_variance != "small", clip=clip_denoised, out=(vb, mse), scratch=scratch)
        finally:
            if was:
                self.denoise_fn.train(True)
        prior = ops.nll_prior(y_0, self.gammas, scratch=scratch)
        return {"total_bpd": prior + vb.sum(dim=1), "prior_bpd": prior, "vb": vb, "x0_mse": mse,
                "eps_mse": mse * plan["snr"], "tau": plan["tau"]}

    # -- the analytic variance: the statistic -----------------------------------------------------
    def _eps_plan_for(self, tau, dev):
        """The device side of a moment estimation: the fp32 tables of schedule.eps_tables, `tau` as int64 and `level`
        = the fp32 `gammas` buffer gathered at tau.  The last plan is kept (estimate_moments asks for the same one per
        batch)."""
        key = (tuple(int(v) for v in tau), self.prediction, dev)
        plan = getattr(self, "_eps_plan", None)
        if plan is None or plan[0] != key:
            tab = _schedule.eps_tables(self.betas64, tau, self.prediction)
            new = {k: torch.tensor(v, dtype=torch.float32, device=dev) for k, v in tab.items()}
            new["tau"] = torch.tensor(list(key[0]), dtype=torch.int64, device=dev)
            new["level"] = self.gammas[new["tau"]].contiguous()
            plan = self._eps_plan = (key, new)
        return plan[1]

    def _check_moments(self, dev, guidance=None, threshold=None, guidance_rescale=None):
        """ValueError, before any launch, where the moments cannot be estimated (eps_moments,
        drivers.estimate_moments): `dev` is where the targets live."""
        if guidance is not None or threshold is not None or \
                (guidance_rescale is not None and float(guidance_rescale) > 0):
            raise ValueError("eps_moments takes no guidance / threshold / guidance_rescale: the moments are those of the "
                             "conditional model's own raw prediction (DESIGN 8)")
        if self._self_cond_p is not None:
            raise ValueError("the moments of a self-conditioned model are not built (DESIGN 8): its prediction depends "
                             "on the chain's own history")
        if torch.device(dev).type != "cuda" or self.gammas.device.type != "cuda":
            raise ValueError("eps_moments runs on the GPU only (the moment is a HIP kernel): move the model and the "
                             "batch there")

    @torch.no_grad()
    def eps_moments(self, y_cond, view_count, angle, y_0, noise=None, seed=None, sample_ids=None, levels=None,
                    guidance=None, threshold=None, guidance_rescale=None):
        """The statistic of the analytic variance (Analytic-DPM; csrc/diffusion.hip holds the definition): per sample
        and level the second moment of the model's noise estimate, m2[b, k] = mean over 3 H W of eps_hat(y_k)^2 with
        eps_hat = ea[k] y_k + eb[k] out_b for the model's own prediction (eps: `out_b` itself; no clamp) and y_k one
        noisy version of the target y_0 at the level gammas[tau[k]].  The loop of bound_terms: for every level -- all T
        (levels=None), K evenly strided ones, or an explicit sequence (schedule.sample_timesteps) -- the bound's noisy
        target (noise (B, K, 3, H, W) wins; else seed= draws it from the counter-based generator, kind 6, keyed by
        sample_ids and the model timestep: use another seed than for the bound on the same images; else torch's device
        generator), one no-grad forward on the inference path and the moment kernel.  A nine-channel network's channels
        6..8 are ignored.  Returns {"m2" (B, K), "tau" (K,)}: device tensors, no host sync inside the loop; launched
        eagerly.  drivers.estimate_moments averages it into M[t].  Refused with ValueError before any launch: guidance /
        threshold / guidance_rescale, a self-conditioned model, a CPU model."""
        from . import ops
        dev = y_0.device
        self._check_moments(dev, guidance, threshold, guidance_rescale)
        b, _, H, W = y_0.shape
        T = self.num_timesteps
        tau = list(range(T)) if levels is None else _schedule.sample_timesteps(T, levels).tolist()
        K = len(tau)
        if noise is not None and tuple(noise.shape) != (b, K, 3, H, W):
            raise ValueError(f"noise must have shape {(b, K, 3, H, W)}, got {tuple(noise.shape)}")
        if tuple(y_cond.shape[-2:]) != (H, W) or y_cond.shape[0] != b:
            raise ValueError(f"y_cond {tuple(y_cond.shape)} does not go with y_0 {tuple(y_0.shape)}")
        plan = self._eps_plan_for(tau, dev)
        ids = None if seed is None or noise is not None else ops.sample_ids(dev, b, sample_ids)
        off, S, _ = ops.view_offsets(view_count, dev)
        y_0, y_cond, angle = y_0.contiguous(), y_cond.contiguous(), angle.contiguous()
        w_on = bool(self.weighting_inference)
        kidx = torch.zeros(b, device=dev, dtype=torch.int64)
        m2 = torch.zeros(b, K, device=dev, dtype=torch.float32)
        scratch = ops.nll_scratch(b, dev)
        y_k = torch.empty_like(y_0)
        draw = dict(noise=noise.contiguous()) if noise is not None else dict(seed=seed, ids=ids)
        z = zero = None
        if noise is None and seed is None:                       # torch's device generator: one level's draw at a time
            z = torch.empty(b, 1, 3, H, W, device=dev, dtype=torch.float32)
            zero = torch.zeros(b, device=dev, dtype=torch.int64)
        x = None
        was = self.denoise_fn.training if isinstance(self.denoise_fn, nn.Module) else None
        if was:
            self.denoise_fn.eval()
        try:
            for k in reversed(range(K)):
                kidx.fill_(k)
                if z is not None:
                    ops.nll_noisy(y_0, zero, plan["tau"][k:k + 1], self.gammas, noise=z.normal_(), out=y_k)
                else:
                    ops.nll_noisy(y_0, kidx, plan["tau"], self.gammas, out=y_k, **draw)
                x, out = self._denoise(y_k, y_cond, angle, kidx, off, S, x=x, copy_cond=x is None, levels=plan["level"])
                ops.eps_moments(out, off, y_k, kidx, plan, b, w_on, out=m2, scratch=scratch)
        finally:
            if was:
                self.denoise_fn.train(True)
        return {"m2": m2, "tau": plan["tau"]}

    # -- training ---------------------------------------------------------------------------
    def forward(self, y_cond, view_count, angle, y_0=None, noise=None, generate=False, t=None, u=None, y_t=None,
                z_seq=None, use_graph=None, seed=None, sample_ids=None, sample_steps=None, solver="ddim", eta=0.0,
                guidance=None, cond_drop=None, threshold=None, threshold_max=None, guidance_rescale=None, distill_z=None,
                distill_level=None, distill_eps=None, distill_x0=None, self_cond=None, variance=None):
        if generate:                      # generate() wrapped in forward for DDP, as in the reference
            return self.generate(y_cond, view_count, angle, y_t=y_t, z_seq=z_seq, use_graph=use_graph, seed=seed,
                                 sample_ids=sample_ids, sample_steps=sample_steps, solver=solver, eta=eta,
                                 guidance=guidance, threshold=threshold, threshold_max=threshold_max,
                                 guidance_rescale=guidance_rescale, variance=variance)
        if variance is not None:
            raise ValueError("variance= belongs to sampling (generate=True): a training step has no reverse variance")
        from . import ops
        b = y_0.shape[0]
        dev = y_0.device
        level = None
        if self._lv_weight is not None:
            self._check_lv(dev)
            if distill_z is not None or self_cond is not None:
                raise ValueError("a distillation or self-conditioned step on a learned-variance model is not built "
                                 "(DESIGN 8)")
        if distill_z is not None or (self._distill is not None and self.training):
            # progressive distillation (set_distill): the teacher phase -- or its four outputs, injected -- then the
            # student's ordinary stacking of z_t at its level, the UNet and the ordinary objective on (eps~, x~)
            tgt = dict(distill_z=distill_z, distill_level=distill_level, distill_eps=distill_eps, distill_x0=distill_x0)
            if self._self_cond_p is not None or self_cond is not None:
                raise ValueError("a distillation step on a self-conditioned model is not built (DESIGN 8)")
            if distill_z is None:
                if cond_drop is not None or u is not None:
                    raise ValueError("a distillation step takes no cond_drop= / u=: its level is gammas[tau_S[i]]")
                tgt = self.distill_targets(y_cond, view_count, angle, y_0, noise=noise, t=t, seed=seed,
                                           sample_ids=sample_ids)
            elif any(v is None for v in tgt.values()):
                raise ValueError("distill_z / distill_level / distill_eps / distill_x0 (distill_targets) come together")
            level = tgt["distill_level"].reshape(-1)
            off, S, max_v = ops.view_offsets(view_count, dev)
            self.last_cond_drop = None
            x, level_s, angle_s = ops.stack_views(y_cond, tgt["distill_z"].contiguous(), None, level, angle, off, S)
            out = self.denoise_fn(x, angle_s, level_s, **self._drop_rng(seed, sample_ids, off, max_v, b, dev))
            return self._objective(out, tgt["distill_eps"], tgt["distill_x0"], level, off, b)
        # self-conditioning (set_self_cond): an injected estimate wins and is used as is; else the first pass runs here
        # and hands back the estimate and, unseeded, the draws it used -- the ordinary step below then draws nothing again
        sc_on = self_cond is not None or self._self_cond_p is not None
        if sc_on:
            self._check_self_cond(y_cond.shape[2], dev)
            if self._level_spec is not None:
                raise ValueError("self-conditioning together with a level sampler is not built (DESIGN 8)")
            if self_cond is None:
                first = self.self_cond_targets(y_cond, view_count, angle, y_0, noise=noise, t=t, u=u, cond_drop=cond_drop,
                                               seed=seed, sample_ids=sample_ids)
                self_cond = first["self_cond"]
                t, u, noise = first.get("t", t), first.get("u", u), first.get("noise", noise)
                cond_drop = first.get("cond_drop", cond_drop)
            elif tuple(self_cond.shape) != tuple(y_0.shape):
                raise ValueError(f"self_cond must have y_0's shape {tuple(y_0.shape)}, got {tuple(self_cond.shape)}")
        # conditioning dropout (set_cond_dropout): an injected mask wins; else drawn in training mode when p > 0
        drop_p = self._cond_drop_p if (cond_drop is None and self.training) else 0.0
        drop = cond_drop
        # the level sampler (set_level_sampler) takes part only when t is drawn here
        smp, iw = None, None
        if self._level_spec is not None and t is None:
            smp = self.level_sampler
            if smp is None:
                raise ValueError("the level sampler runs on the GPU only: move the model there and call "
                                 "set_level_sampler again")
        ids = sample_ids
        if seed is not None:              # whatever was not injected comes from the counter-based generator
            ids = ops.sample_ids(dev, b, sample_ids)
            if drop_p > 0:                # word 2 of the call that gives the sample's t and u
                drop = ops.draw_cond_drop(seed, ids, drop_p)
            if smp is not None:           # draw_train's sibling: the same words, t through the proposal table
                t, level_d, u_d, iw = ops.draw_level(smp, self.gammas, seed=seed, ids=ids)
                if u is None:
                    level = level_d
            elif t is None or u is None:
                t_d, level_d, u_d = ops.draw_train(seed, ids, self.gammas, want_u=t is not None)
                if t is None and u is None:
                    t, level = t_d, level_d
                elif t is None:
                    t = t_d
                else:
                    u = u_d
            if noise is None:             # a launch of its own in front of the stacking kernel (which is unchanged)
                noise = ops.randn_ids(seed, ids, ops.diffusion.RNG_TRAIN_NOISE, 0, tuple(y_0.shape[1:]))
        # same draw order as the reference: t, u, noise
        if t is None and smp is not None:     # one 32-bit word per sample where randint draws t
            t, _, _, iw = ops.draw_level(smp, self.gammas, words=torch.randint(0, 2 ** 32, (b,), device=dev))
        if t is None:
            t = torch.randint(1, self.num_timesteps, (b,), device=dev).long()
        if u is None and level is None:
            u = torch.rand((b, 1), device=dev)
        if noise is None:
            noise = torch.randn_like(y_0)
        if drop is None and drop_p > 0:   # after t, u and noise: the reference's draw order for those is unchanged
            drop = torch.rand(b, device=dev) < drop_p
        if level is None:
            level = ops.gather_level(self.gammas, t, u.reshape(-1).contiguous())
        off, S, max_v = ops.view_offsets(view_count, dev)
        if drop is not None:
            drop = ops.diffusion._drop_mask(drop, b, dev)
        self.last_cond_drop = drop
        sc = {} if not sc_on else dict(self_cond=None if self_cond is None else self_cond.contiguous(), sc_channels=True)
        x, level_s, angle_s = ops.stack_views(y_cond, y_0.contiguous(), noise.contiguous(), level, angle, off, S,
                                              drop=drop, **sc)
        out = self.denoise_fn(x, angle_s, level_s, **self._drop_rng(seed, ids, off, max_v, b, dev))
        return self._objective(out, noise, y_0, level, off, b, smp, iw, t)

    def _drop_rng(self, seed, sample_ids, off, max_views, b, dev):
        """The keyword that keys the UNet's residual-block Dropout masks by (seed, sample id, view, layer)
        (UNet.forward, drop_rng): only with seed=, in training mode and when denoise_fn is our UNet with dropout > 0.
        Anything else -- a foreign denoise_fn(x, angle, level) above all -- is called as before."""
        from .unet import UNet
        fn = self.denoise_fn
        if seed is None or not self.training or not (isinstance(fn, UNet) and fn._has_dropout()):
            return {}
        from . import ops
        return {"drop_rng": (seed, ops.sample_ids(dev, b, sample_ids), off, max_views)}

    def _objective(self, out, noise, y_0, level, off, b, smp=None, iw=None, t=None):
        """The training loss of the composed output against (noise, y_0) at `level`: the reference's MSE, or the
        loss-option kernels (set_loss, loss_hist, a level sampler, a prediction other than "eps")."""
        from . import ops
        self.last_t, self.last_importance_weight = (None, None) if smp is None else (t, iw)
        if self._loss is None and self.loss_hist is None and smp is None and self.prediction == "eps" and \
                self._lv_weight is None:
            return ops.compose_mse_loss(out, noise, off, b, bool(self.weighting_train))
        # "v" / "x0": the loss kernels form the target themselves, from the noise and y_0
        pred = {} if self.prediction == "eps" else dict(prediction=self.prediction, y_0=y_0)
        if self._lv_weight is not None:   # the hybrid objective: the same launch count, one more per-sample output
            loss, sample_loss, _, vlb = ops.compose_loss(
                out, noise, off, b, bool(self.weighting_train), level, **(self._loss or {}), hist=self.loss_hist,
                want_weight=True, vlb=(t.reshape(-1).to(torch.int64).contiguous(), *self._lv_tables(), self._lv_weight),
                **pred)
            self.last_sample_loss, self.last_level = sample_loss.detach(), level.detach()
            self.last_sample_vlb = vlb.detach()
            return loss
        loss, sample_loss, weight = ops.compose_loss(out, noise, off, b, bool(self.weighting_train), level,
                                                     **(self._loss or {}), hist=self.loss_hist, sample_scale=iw,
                                                     want_weight=True, **pred)
        self.last_sample_loss, self.last_level = sample_loss.detach(), level.detach()
        if smp is not None and smp.kind == "loss_aware" and self.training:
            ops.level_stats(smp, self.last_sample_loss, weight.detach(), t)
        return loss
