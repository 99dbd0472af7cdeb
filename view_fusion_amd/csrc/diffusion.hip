// ViewFusion glue around the UNet: ragged view stacking (+ q_sample), softmax-over-views
// noise composition (+ MSE and its backward), and the fused reverse-diffusion step tail.
// Reference: model/view_fusion.py:162-164 (q_sample), :244-263 / :95-115 (stacking),
// :265-298 / :116-150 (compose / mean ablation / loss), :70-84,152-177 (posterior, p_sample).
//
// All HBM-bound and tiny next to the UNet; their point is that NOTHING here needs a host
// sync: ragged view counts come in as a device prefix-sum array `off[B+1]`.
//
// A map of this file, in the order of the file:
//   stacking        stack_views_kernel (on the training step) and stack_views_cfg_kernel<SC>, the same kernel with
//                   conditioning dropout and null rows, and with SC the third part of self-conditioning -- the plain one
//                   stands apart on purpose: behind a shared body the compiler generates other code for it
//                   (profiles/tail_templates.md; the two guided flavours as one template: profiles/loss_lv_templates.md);
//                   draw_cond_drop_kernel.
//   composition     compose4 (softmax over the views, or the mean), guide4, write_weights (the softmax weights handed
//                   back by the tails; compose_fwd_kernel and compose_eps_kernel keep that loop written out, for the
//                   same reason).
//   training loss   compose_fwd / loss_finish / compose_mse_bwd: the MSE pair of the benchmarked step.  It stands apart from
//                   the family below on purpose: with the chain-rule block of compose_mse_bwd_kernel in a __device__
//                   function shared with the family, that kernel's code changes (SGPR 47 -> 45, s_add_u32 / s_addc_u32
//                   4 -> 3: scalar address arithmetic associated differently; profiles/loss_templates.md), and the three
//                   kernels of the benchmarked step keep their code.
//   the loss family pred_target4, compose_loss_fwd_kernel<PEN, PRED, LV> -> compose_loss_finish_kernel, and
//                   compose_loss_bwd_kernel<PEN, PRED, LV>: every other objective.  PEN: the penalty (mse / l1 / huber);
//                   PRED: what channels 0..2 mean -- eps (the target handed over ready-made), v, x0 (the target formed in
//                   registers from noise, y_0 and level); LV: the hybrid loss of a learned variance -- three variance
//                   channels and a KL term taken in registers on the same residual (compose4_var, VlbArgs, vlb_sample in
//                   front of the family; vlb.h holds the arithmetic); eighteen instantiations of each.  The finish kernel
//                   takes the prediction's native noise-level weight (none / min-SNR / P2 / truncated SNR) at run time, an
//                   optional per-sample scale (the importance weight of a level-sampler draw) or, never both, the vlb
//                   partials and lambda, and writes the per-sample loss and an optional loss-by-level histogram.  Same
//                   launch count as the MSE pair, no atomics; loss_weight.h holds the specification.  The tails have no
//                   such switch: another parameterisation is another (a, b) table pair.
//   step arithmetic y0_hat, y0_hat_as, posterior_update, multistep_base / _add: how each product and sum of a reverse
//                   step is rounded, and why it is written operation by operation; EpsBound / EpsBuffer: what a tail on
//                   the eps buffer knows about its sample.
//   the tails       p_sample_tail_kernel<CFG, EPS, RNG> (ancestral: the one-step DDPM posterior) and
//                   sampler_step_kernel<CFG, EPS, RNG> (few-step: a table-driven linear-multistep update, strided DDIM /
//                   DPM-Solver++ 2M).  Three switches: CFG -- the composed eps is guided by the sample's null row; EPS --
//                   eps is read back from the composed-eps pass (rescaled, dynamically thresholded) instead of composed
//                   here, which implies !CFG; RNG -- z is drawn in the kernel (rng.h: Philox4x32-10 keyed by seed and a
//                   per-sample id) instead of loaded.  Six instantiations of each.  In front of them the two noise sources
//                   (load_z, draw_z) and the common prologue (tail_sample, tail_eps).
//   draws, metrics  draw_train, randn_ids, philox_ids (rng.h), gather_level, psnr.
//   level sampling  draw_level_kernel, level_stats_kernel: importance-sampled timesteps from a proposal table the loss
//                   statistics rebuild on the device (level_sampler.h); the draw's weight is the loss family's scale.
//   three launches  compose_eps_kernel<CFG, FUSED_TAIL> -> sample_stat_kernel (abs_select, quantile_lerp; the same
//                   selection on a plain buffer: abs_quantile_kernel) -> an EPS tail: the thresholded / rescaled step.
//   distillation    distill_begin_kernel (the draw of i, z_t) and distill_target_kernel<CFG> (the second teacher step's tail:
//                   x2, x~, eps~), siblings of draw_train / stack_views and of sampler_step_kernel.
//   self-conditioning  self_cond_estimate_kernel<PRED> (the first pass's clamped x0 estimate) and draw_self_cond_kernel:
//                   siblings, behind the distillation pair; its stacking is stack_views_cfg_kernel<true>, above.
//   learned variance  sampler_step_lv_kernel<CFG, RNG> (the few-step tail with a per-pixel noise scale; it rounds the guided
//                   combination and the base otherwise than sampler_step_kernel and has no history term, so it stays a
//                   sibling), behind the self-conditioning kernels; the hybrid loss is the loss family's LV switch, above.
//   the bound       nll_noisy_kernel<RNG>, nll_term_kernel<LV, DEC>, nll_prior_kernel, nll_finish_kernel: the terms of the
//                   variational bound in bits per dimension (evaluation only), behind the loss family's launch tables.
//   analytic variance  eps_moment_kernel (nll_term_kernel's sibling; its finish step is nll_finish_kernel): the second
//                   moment of the recovered noise per (sample, level), behind the bound's kernels.
//   C ABI           one extern "C" entry point per path (include/vf_hip.h).  The twelve tail entries vf_p_sample_tail* /
//                   vf_sampler_step* {"", _cfg, _eps} x {"", _rng} each name one instantiation and forward to the one
//                   launcher of their flavour (p_sample_tail, sampler_step), which holds the argument check.  The seven
//                   vf_compose_loss_* entries (the two _lv_ ones among them) likewise forward to loss_fwd / loss_bwd;
//                   loss_kernels<LV> turns the run-time (penalty, pred) into the instantiation.
// With every option off a path runs the launches and the bits it ran before the option existed.
//
// Classifier-free guidance (Ho & Salimans, "Classifier-Free Diffusion Guidance").  This comment is the ONE written
// definition; tests/guidance_ref.py restates it.  Opt-in: siblings of the kernels above, which are untouched.
//   Null conditioning.  The unconditional input of sample b is its own noisy target next to an all-zero conditioning half
//     (all Cc channels, 3 or 6); its own level and angle (the relative angle in the `relative` configs) are kept.
//   Guided noise.  eps = g_b * eps_c + (1 - g_b) * eps_u, in this order with 1 - g_b formed first, so that g = 1 gives
//     eps_c and g = 0 gives eps_u exactly, contracted to a multiply-add or not.  eps_c: the composition over the sample's
//     real views (softmax-weighted, or the mean) as above; eps_u: noise channels 0..2 of the sample's null row (that
//     row's logit channels are ignored); g_b: a per-sample fp32 scale read from device memory (g > 1 extrapolates).
//     The weights handed back stay the conditional softmax weights.
//   Rows of a guided step.  The stacked batch has S + B rows: rows 0..S-1 are the unguided step's, under the same `off`
//     table, and row S + b (S = off[B]) is sample b's null row.  Nothing that reads `off` changes meaning.
//   Training drop (seeded; rng.h).  Sample `id` is dropped iff (w2 >> 8) < thr, w2 = word 2 of the kind-0, step-0, block-0
//     call that already gives t (word 0) and u (word 1), thr = ceil(p * 2^24) computed on the host: an integer compare.
//     p = 1 drops every sample; p = 0 is "off" and launches nothing.
//   A dropped sample keeps its view_count: ALL its rows get the zero conditioning half, so S, `off` and every shape stay
//     static for a captured step.  Its rows are then identical, so the composition (a convex combination) returns that one
//     prediction -- the prediction of the single null row that sampling uses.
//
// Dynamic thresholding (Saharia et al., Imagen, 2.3) and guidance rescaling (Lin et al., "Common Diffusion Noise
// Schedules and Sample Steps are Flawed", 3.4) for the reverse step.  This comment is the ONE written definition;
// tests/threshold_ref.py restates it.  Opt-in: with both off every path runs the kernels above, untouched.
//   n = 3 H W; every statistic is per sample b, over its n elements.
//   1. eps_c = the composed noise (softmax over views, or the mean); eps_g = g eps_c + (1 - g) eps_u when guided, else
//      eps_g = eps_c: compose4 / guide4 as above.
//   2. Rescale (phi in (0, 1], needs guidance): r_b = phi (sigma(eps_c) / sigma(eps_g)) + (1 - phi), sigma the standard
//      deviation over the n elements (the same n in both, so n against n - 1 cancels); r_b = 1 where sigma(eps_g) == 0;
//      eps = r_b eps_g.  Off: eps = eps_g, no multiply.
//   3. y0_hat = a y - b eps with the step's own table pair (sqrt_recip_gammas[t], sqrt_recipm1_gammas[t]; a[k], b[k]).
//   4. Threshold (q in (0, 1], optional cap c >= 1): x = sort(|y0_hat|), pos = q (n - 1) in float64 on the host,
//      k = floor(pos), frac = float32(pos - k); s_q = x[k] + frac (x[k+1] - x[k]) (torch.quantile's linear interpolation;
//      x[k+1] is not read when frac == 0, which covers q = 1); s_b = max(1, s_q), then min(s_b, c);
//      y0 = clamp(y0_hat, -s_b, s_b) / s_b.  This replaces the static clamp.  Off: the static clamp stays as it is.
//   5. The rest of the step is unchanged (posterior mean + z sd, or cy y + c0 y0 + c1 y0_prev + sigma z); y0_prev
//      receives the thresholded y0.     6. Weights and logits stay the conditional ones.
//   NaN / Inf inputs: unspecified.
//   Three launches instead of the one tail: compose_eps_kernel writes eps_g, the weights and per-workgroup partial sums
//   of eps_c, eps_c^2, eps_g, eps_g^2 (doubles, fixed-order trees, no atomics on global memory); sample_stat_kernel, one
//   workgroup per sample, adds the partials in index order (double) -> r_b, then finds x[k] and x[k+1] of
//   |a y - b r_b eps_g| EXACTLY by radix selection on the bit pattern with the sign cleared -- monotone for non-negative
//   floats, denormals and -0 included -- with LDS histograms of 32-bit integer counts (integer adds commute, so LDS
//   atomics do not make the result depend on their order), and writes stat[b] = {r_b, s_b}; the *_eps tails read eps_g and
//   stat.  t / kidx / stat all live in device memory: a captured step replays for every step.
//
// Prediction: what channels 0..2 of the network mean (Salimans & Ho, "Progressive Distillation", v; Hang et al., Min-SNR,
// the weights).  This comment is the ONE written definition (the weights: loss_weight.h); tests/prediction_ref.py
// restates it.  One switch (PRED) of the loss family: "eps" is handed its target ready-made and computes the bits it
// computed before the switch existed.
//   g = the level the network is conditioned on: the sample's continuous `level` in training, gammas[t] / gammas[tau[k]]
//   in sampling.  y_t = sqrt(g) y_0 + sqrt(1 - g) noise as before.  `out` = the composition over the sample's views of
//   channels 0..2 (softmax of channels 3..5, or the mean), unchanged: the weights sum to 1 and everything below is affine
//   in `out` with the same y_t in every view, so composing the views' outputs equals composing their noise estimates, and
//   guiding `out` (g out_c + (1 - g) out_u) equals guiding eps.
//     prediction   training target                       y0_hat = a y - b out                 c(g)
//     "eps"        noise                                 a = g^-1/2, b = (1/g - 1)^1/2        1
//     "v"          sqrt(g) noise - sqrt(1 - g) y_0       a = sqrt(g), b = sqrt(1 - g)         g
//     "x0"         y_0                                   a = 0,       b = -1  (y0_hat == out)  g / (1 - g)
//   c(g): the native weight per unit of epsilon-equivalent weight (loss_weight.h).  The penalties, the per-sample loss, the
//   histogram, the level sampler's importance weight and its (w s)^2 statistic are taken on the native residual.
//   Guidance rescaling takes sigma of the composed output in the network's own parameterisation (Lin et al.); the
//   threshold acts on y0_hat.  Everything after y0_hat (posterior, multistep update, threshold, y0_prev) uses y0 alone:
//   sampling in another parameterisation hands the tails another (a, b) table pair, and no tail kernel changes.
//   With gamma_T = 0 (a zero-terminal-SNR schedule) the "eps" pair is infinite there; the "v" and "x0" pairs are finite.
//
// Progressive distillation (Salimans & Ho, "Progressive Distillation for Fast Sampling of Diffusion Models"): the target
// of a student that does in one deterministic DDIM step what its teacher does in two.  This comment is the ONE written
// definition; tests/distill_ref.py restates it.  Opt-in: two sibling kernels, everything above is untouched.
//   Grids.  K >= 1 student steps with 2K <= T: tau_S = sample_timesteps(T, K), tau_T = sample_timesteps(T, 2K), so that
//     tau_T[2i+1] == tau_S[i], and step 0 of both lands on the clean image.
//   Tables.  Teacher: sampler_tables(betas, tau_T, "ddim", 0, teacher.prediction) -> a_T, b_T, cy_T, c0_T.  Student:
//     sampler_tables(betas, tau_S, "ddim", 0) -> cy_S, c0_S.  w1[i] = cy_T[2i] c0_T[2i+1] / c0_S[i], w2[i] = 1 - w1[i],
//     formed in float64 on the host and rounded to fp32 once (schedule.distill_tables); 0 <= w1 <= 1 and w1[0] = 0.
//   For sample b with student step i = i_b in 0..K-1:
//   1. g = gammas[tau_S[i]] (the fp32 buffer value: the level the student's own K-step sampler conditions it on);
//      z_t = sqrt(g) y_0 + sqrt(1 - g) noise, stack_views_kernel's expression.                       [distill_begin_kernel]
//   2. Teacher step k1 = 2i + 1 at level gammas[tau_T[k1]], the existing sampler_step with a history buffer:
//      x1 = clamp(a_T[k1] z_t - b_T[k1] out1, -1, 1) -> the history buffer;  z' = cy_T[k1] z_t + c0_T[k1] x1.
//      out1: the composition of the teacher's output over the sample's views, guided by its null row when guidance is set.
//   3. Teacher step k0 = 2i on the teacher's output at z', level gammas[tau_T[k0]]:
//      x2 = clamp(a_T[k0] z' - b_T[k0] out2, -1, 1), rounded as sampler_step_kernel rounds y0.     [distill_target_kernel]
//   4. x~ = clamp(fma(w1[i], x1, w2[i] x2), -1, 1): a convex combination of two clamped predictions -- the clamp only takes
//      back a last place by which fp32 w1 + w2 may exceed 1; with i = 0 (w1 = 0, w2 = 1) x~ is x2 bit for bit.  This is the
//      paper's x~ = (z'' - (sigma''/sigma) z_t) / (alpha'' - (sigma''/sigma) alpha_t) without its cancellation: cy_S =
//      cy_T[2i] cy_T[2i+1] and cy_T[2i] c0_T[2i+1] + c0_T[2i] = c0_S[i], so cy_S z_t + c0_S x~ is the teacher's z''.
//   5. eps~ = (z_t - sqrt(g) x~) / sqrt(1 - g), every operation rounded, in this order.
//   6. The student sees z_t and g bit for bit; its loss is the existing objective with noise := eps~ and y_0 := x~ (the loss
//      kernels then form its native target themselves: eps~, sqrt(g) eps~ - sqrt(1 - g) x~, or x~).
//   The draw of i (seeded): i_b = mulhi32(w0, K), w0 = word 0 of the sample's kind-0 call (where t comes from otherwise);
//   an injected i is clamped to 0..K-1 before any table is read.  i, k1, k0 (int64), g, tables and weights live in device
//   memory: a captured phase replays for every step.  No EPS / threshold / rescale flavour.
//
// Self-conditioning (Chen et al., "Analog Bits", 2.2): the network is also shown its own previous estimate of the clean
// image.  This comment is the ONE written definition; tests/selfcond_ref.py restates it.  Opt-in: the SC instantiation of
// the guided stacking kernel (stack_views_cfg_kernel<true>) and two sibling kernels (self_cond_estimate_kernel<PRED>,
// draw_self_cond_kernel); every path without it runs the code it ran before.
//   Input.  UNet(in_channel = Cc + 6): row v of sample b is [ cond (Cc) | noisy target (3) | sc_b (3) ], Cc = 3 or 6 as
//     before; sc_b is the same in all the sample's rows; under guidance the null row S + b is [ 0 | y_b | sc_b ];
//     sc_b = 0 means "no estimate".  The first Cc + 3 channels are stack_views_cfg_kernel<false>'s expressions.
//   Estimate (training; g = level[b], the sample's continuous level; out_b = the composition over the sample's views of
//     channels 0..2 under weighting_train: compose4, softmax of channels 3..5 or the mean):
//       x^_b = keep_b clamp(a(g) y_t - b(g) out_b, -1, 1)
//     with y_t READ BACK from the target part of the stacked input the first pass saw (stack_views_kernel's q_sample
//     expression, so its bits), and, in fp32,
//       eps   a = sqrtf(1 / g),  b = sqrtf((1 - g) / g)    ( = sqrt(1 / g - 1) without its cancellation at g -> 1: 1 - g is
//                                                            exact for g >= 1/2, so b is within 2 ulp for every level)
//       v     a = sqrtf(g),      b = sqrtf(1 - g)
//       x0    a = 0, b = -1: x^ = clamp(out) to the bit -- y_t is not read and nothing is multiplied.
//     Rounding: a y_t and b out_b are each rounded, then subtracted (y0_hat_as<false>, as sampler_step_kernel forms y0),
//     then clamped; keep_b = 0 writes exact zeros and reads nothing of `out`.  vf_self_cond_coeffs (below) is the one copy
//     of (a, b); vf_self_cond_coeffs_host runs it on the CPU.
//   Coin.  keep_b = 1 with probability p, per sample.  Seeded: keep = (w3 >> 8) < thr, thr = ceil(p 2^24) on the host, w3 =
//     word 3 of the kind-0, step-0, block-0 call that gives t (word 0), u (word 1) and the conditioning drop (word 2): an
//     integer compare and a function of (seed, sample id) alone.  p = 0 launches nothing extra; p = 1 keeps every sample.
//   Training step.  Pass 1, no gradient, no Dropout: the stacked input with zero sc channels (same y_t, level, angle and
//     conditioning-drop mask as pass 2) -> out -> x^.  Pass 2: the ordinary step on the input whose sc channels hold x^.
//     Samples with keep = 0 still run pass 1 (static shapes).  The objective is unchanged.
//   Sampling.  sc = the history buffer sampler_step_kernel writes (y0_prev: the step's final y0 -- clamped or thresholded,
//     guided), zero before the first step; the stacking kernel reads it at the top of a step, the tail overwrites it at the
//     end.  With dpmpp2m the tail reads the same buffer as its own history: both want the previous step's y0.
//
// Learned variance (Nichol & Dhariwal, "Improved DDPM", 3.1 and 4): the network also predicts, per pixel, where between
// log beta~ and log beta the log-variance of a reverse step lies, and is trained with L_simple + lambda L_vlb.  This
// comment is the ONE written definition (the arithmetic, operation by operation: vlb.h); tests/vlb_ref.py restates it.
// Opt-in: the LV instantiations of the loss family (compose_loss_fwd_kernel / _bwd_kernel<PEN, PRED, true>, the vlb
// operands of compose_loss_finish_kernel) and a sibling tail (sampler_step_lv_kernel<CFG, RNG>); every path without it runs
// the code it ran before.
//   Network.  UNet(out_channel = 9): channels 0..2 the prediction (eps, v or x0) and 3..5 the view logits as before, 6..8
//     the raw variance output o.  o_b = the composition over the sample's real views of channels 6..8 under the weights of
//     channels 0..2 (the softmax of 3..5, or the mean).  v = 0.5 o_b + 0.5, unconstrained;  lp = v hi + (1 - v) lo, every
//     operation rounded in this order, no fused multiply-add.
//   Tables (schedule.variance_tables, float64, rounded to fp32 once).  For a chain tau (default 0..T-1), gt = gammas[tau[k]],
//     gp = gammas[tau[k-1]] (1 at k = 0):  hi[k] = log(1 - gt/gp),  lo[k] = log(max((1 - gt/gp)(1 - gp)/(1 - gt), 1e-20));
//     on the full schedule hi = log(betas) and lo = posterior_log_variance_clipped, value for value.
//   Training term.  Sample b: timestep t in 1..T-1, continuous level g, r = the native residual the loss family forms
//     (composed prediction - pred_target4), a CONSTANT inside the vlb term: it carries no gradient there.
//       m^2 = c1[t]^2 kappa^2(g) r^2, c1 = posterior_mean_coef1; kappa^2 = (1 - g)/g (eps) | 1 - g (v) | 1 (x0): the squared
//             distance of the posterior means, (mu~ - mu_theta)^2, with y0_hat = a(g) y_t - b(g) out unclamped;
//       KL  = 0.5 (-1 + lp - lo[t] + exp(lo[t] - lp) + m^2 exp(-lp)) / ln 2;
//       vlb_b = the mean of KL over the sample's 3 H W elements, in bits per dimension;
//       loss = L_simple + lambda (1/B) sum_b vlb_b.
//     L_simple is the loss family's objective, unchanged: penalties, the noise-level weight, the per-sample loss and the
//     histogram, all on r.  The vlb term takes no SNR weight.  t is never 0 in training (draw_train gives 1..T-1), so the
//     discretised decoder likelihood of t = 0 takes no part in training; the evaluation of the bound builds it
//     ("Variational bound", below).
//   Gradient.  dloss/dlp = (lambda / (n B)) 0.5 (1 - exp(lo - lp) - m^2 exp(-lp)) / ln 2;  dlp/do_b = 0.5 (hi - lo);
//     channels 6..8 get w_v g, the logits 3..5 get w_v (o_v - o_b) g ADDED to L_simple's logit gradient, channels 0..2 get
//     L_simple's gradient only; mean ablation: channels 6..8 get g / count, the logits 0.
//   Sampling step (the table-driven tail on the "ddim", eta = 1 tables, whose mean is the posterior mean):
//     y0 = clamp(a[k] y - b[k] out, -1, 1);  r = cy[k] y + c0[k] y0, both rounded as sampler_step_kernel<CFG, false, RNG>
//     rounds them;  where sigma[k] != 0 (every step but k = 0): r += expf(0.5f lp) z with lp from hi[k], lo[k] and o_b;
//     y0_prev <- y0 when a history buffer is passed.  Weights, logits and the draw of z (step = tau[k]) are that kernel's.
//     Guided: `out` is guided as before; o_b comes from the CONDITIONAL rows only, the null row's channels 6..8 are
//     ignored (GLIDE).  No EPS / threshold / rescale flavour.
//
// Variational bound (Ho et al., DDPM, eq. 5; Nichol & Dhariwal, "Improved DDPM", 2.3 and calc_bpd_loop): the bound on
// -log2 p(y_0) of held-out targets, in bits per dimension, term by term.  This comment is the ONE written definition (the
// arithmetic, operation by operation: vlb.h and nll_element below); tests/nll_ref.py restates it.  Opt-in and additive:
// new kernels only (nll_noisy_kernel<RNG>, nll_term_kernel<LV, DEC>, nll_prior_kernel, nll_finish_kernel), behind the
// loss family's launch tables; nothing above changes.
//   Chain.  tau of K steps (default 0..T-1; schedule.sample_timesteps otherwise), gt = gammas[tau[k]], gp = gammas[tau[k-1]]
//     (1 at k = 0).
//   Noisy target.  Per sample b and step k one Monte-Carlo draw: y_k = sqrt(gt) y_0 + sqrt(1 - gt) n with the fp32 buffer
//     value gt, both products rounded, then added.  n is injected ((B, K, 3, H, W)), or drawn: Philox kind 6 (rng.h),
//     step = tau[k], block = the float4 index, keyed by (seed, sample id).  The network runs on the inference path at
//     the discrete level gt, its rows stacked as generate() stacks them.
//   Model distribution (the sampler's own).  y0 = clamp(a[k] y_k - b[k] out_b, -1, 1) (no clamp under
//     clip_denoised=False); (a, b) = schedule.prediction_tables at tau for eps, v or x0; out_b = compose4 over the sample's
//     real views.  The model's mean minus the true posterior mean is c0[k] (y0 - y_0) with
//     c0[k] = sqrt(gp) (1 - gt/gp) / (1 - gt) (posterior_mean_coef1 on the full chain, value for value): m^2 = c0^2 (y0 - y_0)^2.
//   Log-variance lp.  A nine-channel model with a learned variance: vf_vlb_logvar(o_b, hi[k], lo[k]), o_b = compose4_var.
//     A fixed variance: lp = lo[k] ("small", what the ancestral sampler uses) or hi[k] ("large").
//   Terms.  k >= 1: L_k = the mean over the 3 H W elements of vf_vlb_kl(lp, lo[k], m^2), in bits.  k = 0, the decoder:
//     L_0 = the mean of vf_nll_decoder(y_0, y0, lp): Improved DDPM's discretised Gaussian likelihood with bins of +-1/255,
//     the tanh approximation of Phi, the open-ended bins below -0.999 and above 0.999, every log argument clamped at 1e-12.
//     Its variance row is not lo[0] = log 1e-20 (the clipping the buffers carry, under which the term degenerates):
//     hi_dec = log(1 - gammas[tau[0]]), lo_dec = the log posterior variance of step 1 of the chain (Improved DDPM's
//     posterior_log_variance_clipped[0]; also the row the network has seen at that level, training draws t >= 1); a
//     one-step chain has lo_dec = hi_dec; "large" uses lo_dec at k = 0 as well, as the paper does.
//     Prior: L_T = the mean of 0.5 (-1 - log(1 - gT) + (1 - gT) + gT y_0^2) / ln 2, gT = gammas[T-1]: exactly 0 at gT = 0.
//     total_bpd_b = L_T + sum_k L_k.
//   Diagnostic.  x0_mse[b, k] = the mean of (y0 - y_0)^2; the error of the recovered noise is x0_mse gt / (1 - gt)
//     identically, formed by the driver: no noise buffer reaches the term kernel.
//   Reduction.  Two partial sums per (b, chunk) by block_sum<256>, then one thread per sample adds its partials in index
//     order: no atomics, the same bits on every run and for every batch the sample stands in.
//   Not built: a captured K-step loop, a guided bound, level resampling on L_vlb.
//
// Analytic variance (Bao et al., "Analytic-DPM", ICLR 2022, Theorem 1 and section 5): the KL-optimal variance of the
// reverse step of any chain, for a pretrained six-channel model, without training.  This comment is the ONE written
// definition; tests/analytic_ref.py restates it.  Opt-in and additive: one new kernel (eps_moment_kernel; its finish step
// is nll_finish_kernel, unchanged), behind the bound's kernels; nothing above changes.
//   Chain.  tau of K steps, gt = gammas[tau[k]], gp = gammas[tau[k-1]] (1 at k = 0), as the bound.
//   Noise estimate, per element.  e = ea[k] y_k + eb[k] out_b: each product rounded, then added, contraction off.
//     out_b = compose4 over the sample's real views of channels 0..2 (softmax of 3..5, or the mean); channels 6..8 of a
//     nine-channel output are ignored.  (ea, eb) = schedule.eps_tables at tau, formed in float64 and rounded to fp32 once:
//       eps: (0, 1)      v: (sqrt(1 - g), sqrt(g))      x0: (1 / sqrt(1 - g), -sqrt(g / (1 - g)))
//     so for eps e is `out` to the bit.  No clamp: the theorem is about the model's raw mean.
//   Moment.  m2[b, k] = the mean of e^2 over the sample's 3 H W elements (one block_sum<256> partial per (b, chunk), then
//     one thread per sample adds its partials in index order: no atomics, the same bits on every run and for every batch
//     the sample stands in).  M[t] = the mean of m2 over samples and draws at t = tau[k], in float64, on the host side of
//     the driver (drivers.estimate_moments).  The noisy targets are the bound's (nll_noisy_kernel, Philox kind 6).
//   Optimal variance.  With lambda^2[k] = sigma[k]^2 and c0[k] of schedule.sampler_tables(betas, tau, "ddim", eta) and
//     Mc = clip(M[tau[k]], 0, 1):
//       sigma*^2[k] = lambda^2[k] + c0[k]^2 (1 - gt) / gt (1 - Mc)
//     -- the paper's lambda^2 + (sqrt(bbar_n / a_n) - sqrt(bbar_{n-1} - lambda^2))^2 (1 - bbar_n Gamma_n) in these tables.
//     The clip is the paper's Theorem 2: lambda^2 <= sigma*^2 <= lambda^2 + c0^2 (1 - gt) / gt.  Sampling sets
//     sigma*[0] = 0 (the last step returns its mean).  ValueError for a level with gamma = 0 (0 times inf) and for a NaN
//     (not estimated) moment at a level the chain uses.  All of it float64 on the host (schedule.analytic_sigma2): the
//     reverse step reads sigma*[k] where it read sigma[k], sampler_step_kernel unchanged.
//   Bound.  fixed_variance="analytic": hi[k] = log sigma*^2[k] at eta = 1, where lambda^2 is the chain's posterior variance
//     and c0 is nll_tables' own; hi[0], the decoder row, = log max(sigma*^2[0], exp(lo_dec)); lo[k] stays the true
//     posterior's.  nll_term_kernel runs as it does for "large".
//   Optimal trajectory (section 5).  J(r, s) = log(sigma*^2(r, s) / lambda^2(r, s)) at eta = 1 for a step from s down to
//     r < s; schedule.optimal_trajectory minimises sum_{k >= 1} J(tau[k-1], tau[k]) over strictly increasing tau with
//     tau[0] = first, tau[K-1] = T-1 by dynamic programming in float64.
//   Not built: a captured estimation loop, moments of a guided model, a draw kind of its own (use another seed than for
//     the bound on the same images), SN-DPM.
#include "common.h"
#include "level_sampler.h"
#include "loss_weight.h"
#include "rng.h"
#include "vlb.h"

namespace {

__device__ __forceinline__ int sample_of_view(const int* __restrict__ off, int B, int v) {
    int lo = 0, hi = B;                       // find b with off[b] <= v < off[b+1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// x[v] = [ y_cond[b][v-off[b]] | y_t[b] ]  with optional q_sample on the fly:
//   y_t' = sqrt(level_b) * y_t + sqrt(1-level_b) * noise.
// The conditioning part has Cc channels (3 = an RGB view; 6 = the `relative` configs' view pair,
// experiment.py:274-283 / configs/relative-small-v100-4.yaml:22), the noisy target always 3.
// grid (chunks, S); nc4 = Cc*HW/4 and n4 = 3*HW/4 float4 per image.
__global__ void stack_views_kernel(const float4* __restrict__ y_cond, const float4* __restrict__ y_t,
                                   const float4* __restrict__ noise, const float* __restrict__ level,
                                   const float* __restrict__ angle, const int* __restrict__ off,
                                   float4* __restrict__ x, float* __restrict__ level_s, float* __restrict__ angle_s,
                                   int B, int Nmax, int nc4, int n4, int copy_cond) {
    const int v = blockIdx.y;
    const int b = sample_of_view(off, B, v);
    const int j = v - off[b];
    const float lv = level[b];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        level_s[v] = lv;
        angle_s[v] = angle[b];
    }
    const float sa = sqrtf(lv), sb = sqrtf(1.0f - lv);
    const float4* c = y_cond + ((size_t)b * Nmax + j) * nc4;
    const float4* t = y_t + (size_t)b * n4;
    const float4* z = noise ? noise + (size_t)b * n4 : nullptr;
    float4* o = x + (size_t)v * (nc4 + n4);
    if (copy_cond)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nc4; i += gridDim.x * blockDim.x) o[i] = c[i];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
        float4 y = t[i];
        if (z) {
            const float4 e = z[i];
            y.x = sa * y.x + sb * e.x;
            y.y = sa * y.y + sb * e.y;
            y.z = sa * y.z + sb * e.z;
            y.w = sa * y.w + sb * e.w;
        }
        o[nc4 + i] = y;
    }
}

// stack_views_kernel with conditioning dropout and null rows (classifier-free guidance, see the head of this file), and
// with SC the third part of self-conditioning: row v = [ cond (nc4) | target (n4) | sc_b (n4) ], sc (B,3,HW) | null = zeros.
// drop (uint8[B] | null): the conditioning half of every row of a sample with drop[b] != 0 is zeros; y_cond is not read
// for it.  grid (chunks, rows): rows = S, or S + B with null rows -- row S + b is [ 0 | y_t[b] (| sc_b) ] with level[b],
// angle[b].  The target half is stack_views_kernel's expression, so equal inputs give equal bits, with or without SC.
// copy_cond == 0 rewrites the target (and sc) part only (the per-step re-stack of generate).
template <bool SC>
__global__ void stack_views_cfg_kernel(const float4* __restrict__ y_cond, const float4* __restrict__ y_t,
                                       const float4* __restrict__ noise, const float* __restrict__ level,
                                       const float* __restrict__ angle, const int* __restrict__ off,
                                       const unsigned char* __restrict__ drop, float4* __restrict__ x,
                                       float* __restrict__ level_s, float* __restrict__ angle_s, int B, int Nmax, int nc4,
                                       int n4, int copy_cond, int S, const float4* __restrict__ sc) {
    const int v = blockIdx.y;
    const bool null_row = v >= S;
    const int b = null_row ? v - S : sample_of_view(off, B, v);
    const int j = null_row ? 0 : v - off[b];
    const bool zero = null_row || (drop != nullptr && drop[b] != 0);
    const float lv = level[b];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        level_s[v] = lv;
        angle_s[v] = angle[b];
    }
    const float sa = sqrtf(lv), sb = sqrtf(1.0f - lv);
    const float4* c = y_cond + ((size_t)b * Nmax + j) * nc4;
    const float4* t = y_t + (size_t)b * n4;
    const float4* z = noise ? noise + (size_t)b * n4 : nullptr;
    const float4* s = SC && sc ? sc + (size_t)b * n4 : nullptr;
    float4* o = SC ? x + (size_t)v * (nc4 + 2 * (size_t)n4) : x + (size_t)v * (nc4 + n4);
    if (copy_cond) {
        if (zero)
            for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nc4; i += gridDim.x * blockDim.x)
                o[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        else
            for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nc4; i += gridDim.x * blockDim.x) o[i] = c[i];
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
        float4 y = t[i];
        if (z) {
            const float4 e = z[i];
            y.x = sa * y.x + sb * e.x;
            y.y = sa * y.y + sb * e.y;
            y.z = sa * y.z + sb * e.z;
            y.w = sa * y.w + sb * e.w;
        }
        o[nc4 + i] = y;
        if constexpr (SC) o[nc4 + n4 + i] = s ? s[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// drop[b] = the training drop draw of sample ids[b] (rng.h: word 2 of the training-scalar call against thr)
__global__ void draw_cond_drop_kernel(unsigned long long seed, const long long* __restrict__ ids, unsigned thr,
                                      unsigned char* __restrict__ drop, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t w[4];
    vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
    drop[b] = (unsigned char)vf_rng_cond_drop(w[2], thr);
}

// The guided combination of one float4: g eps_c + (1 - g) eps_u, gm = 1 - g formed by the caller.
__device__ __forceinline__ float4 guide4(float4 ec, const float* __restrict__ eu, float g, float gm) {
    const float4 u = *reinterpret_cast<const float4*>(eu);
    return make_float4(g * ec.x + gm * u.x, g * ec.y + gm * u.y, g * ec.z + gm * u.z, g * ec.w + gm * u.w);
}

// Composed noise for one float4 of (b, c, pixels): softmax over the sample's views of the
// logits (channels 3..5) weighting the per-view noise (channels 0..2); or the plain mean.
__device__ __forceinline__ float4 compose4(const float* __restrict__ out, int Cout, int HW, int v0, int v1, int c,
                                           int p, int weighting, float4* mx_out, float4* inv_out) {
    const size_t vs = (size_t)Cout * HW;
    const float* e0 = out + (size_t)v0 * vs + (size_t)c * HW + p;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!weighting) {
        for (int v = v0; v < v1; ++v) {
            const float4 e = *reinterpret_cast<const float4*>(e0 + (size_t)(v - v0) * vs);
            acc.x += e.x; acc.y += e.y; acc.z += e.z; acc.w += e.w;
        }
        const float inv = 1.0f / (float)(v1 - v0);
        return make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
    }
    const float* l0 = e0 + (size_t)3 * HW;
    float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int v = v0; v < v1; ++v) {
        const float4 l = *reinterpret_cast<const float4*>(l0 + (size_t)(v - v0) * vs);
        mx.x = fmaxf(mx.x, l.x); mx.y = fmaxf(mx.y, l.y); mx.z = fmaxf(mx.z, l.z); mx.w = fmaxf(mx.w, l.w);
    }
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int v = v0; v < v1; ++v) {
        const float4 l = *reinterpret_cast<const float4*>(l0 + (size_t)(v - v0) * vs);
        const float4 e = *reinterpret_cast<const float4*>(e0 + (size_t)(v - v0) * vs);
        const float wx = expf(l.x - mx.x), wy = expf(l.y - mx.y), wz = expf(l.z - mx.z), ww = expf(l.w - mx.w);
        sum.x += wx; sum.y += wy; sum.z += wz; sum.w += ww;
        acc.x += wx * e.x; acc.y += wy * e.y; acc.z += wz * e.z; acc.w += ww * e.w;
    }
    const float4 inv = make_float4(1.0f / sum.x, 1.0f / sum.y, 1.0f / sum.z, 1.0f / sum.w);
    if (mx_out) { *mx_out = mx; *inv_out = inv; }
    return make_float4(acc.x * inv.x, acc.y * inv.y, acc.z * inv.z, acc.w * inv.w);
}

// The softmax weights of float4 i = (c, p) of sample b into weights[B][maxV][3][HW], zero for the views the sample does
// not have; (mx, inv) as compose4 hands them back.
__device__ __forceinline__ void write_weights(const float* __restrict__ out, float* __restrict__ weights, int Cout,
                                              int HW, int maxV, int v0, int v1, int c, int p, int i,
                                              const float4& mx, const float4& inv) {
    const int b = blockIdx.y;
    const size_t vs = (size_t)Cout * HW;
    for (int j = 0; j < maxV; ++j) {
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (v0 + j < v1) {
            const float4 l = *reinterpret_cast<const float4*>(out + (size_t)(v0 + j) * vs + (size_t)(3 + c) * HW + p);
            w = make_float4(expf(l.x - mx.x) * inv.x, expf(l.y - mx.y) * inv.y, expf(l.z - mx.z) * inv.z,
                            expf(l.w - mx.w) * inv.w);
        }
        *reinterpret_cast<float4*>(weights + (((size_t)b * maxV + j) * 3) * HW + 4 * (size_t)i) = w;
    }
}

// grid (chunks, B).  Writes noise_hat[B][3][HW]; optional weights[B][maxV][3][HW] (zero padded);
// optional per-block partial sums of (target - noise_hat)^2 into loss_part[B*chunks].
__global__ __launch_bounds__(256) void compose_fwd_kernel(const float* __restrict__ out, const int* __restrict__ off,
                                                          const float* __restrict__ target,
                                                          float* __restrict__ noise_hat, float* __restrict__ weights,
                                                          float* __restrict__ loss_part, int Cout, int HW, int maxV,
                                                          int weighting) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    float sq = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        float4 mx, inv;
        const float4 nh = compose4(out, Cout, HW, v0, v1, c, p, weighting, &mx, &inv);
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        *reinterpret_cast<float4*>(noise_hat + o) = nh;
        if (target) {
            const float4 t = *reinterpret_cast<const float4*>(target + o);
            const float dx = t.x - nh.x, dy = t.y - nh.y, dz = t.z - nh.z, dw = t.w - nh.w;
            sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
        if (weights && weighting) {
            const size_t vs = (size_t)Cout * HW;
            for (int j = 0; j < maxV; ++j) {
                float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
                if (v0 + j < v1) {
                    const float4 l = *reinterpret_cast<const float4*>(out + (size_t)(v0 + j) * vs +
                                                                     (size_t)(3 + c) * HW + p);
                    w = make_float4(expf(l.x - mx.x) * inv.x, expf(l.y - mx.y) * inv.y, expf(l.z - mx.z) * inv.z,
                                    expf(l.w - mx.w) * inv.w);
                }
                *reinterpret_cast<float4*>(weights + (((size_t)b * maxV + j) * 3) * HW + 4 * (size_t)i) = w;
            }
        }
    }
    if (loss_part) {
        sq = block_sum<256>(sq, red);
        if (threadIdx.x == 0) loss_part[blockIdx.y * gridDim.x + blockIdx.x] = sq;
    }
}

__global__ void loss_finish_kernel(const float* __restrict__ part, float* __restrict__ loss, int n, float scale) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float a = 0.f;
        for (int i = 0; i < n; ++i) a += part[i];
        *loss = a * scale;
    }
}

// d(out) for loss = mean((target - noise_hat)^2) * gloss:
//   g = 2 (nh - target) / n * gloss;  d eps_v = w_v g;  d logit_v = w_v (eps_v - nh) g
// (mean ablation: d eps_v = g / count, logits untouched -> zero).
__global__ __launch_bounds__(256) void compose_mse_bwd_kernel(const float* __restrict__ out,
                                                              const int* __restrict__ off,
                                                              const float* __restrict__ target,
                                                              const float* __restrict__ noise_hat,
                                                              const float* __restrict__ gloss,
                                                              float* __restrict__ dout, int Cout, int HW,
                                                              int weighting, float inv_n) {
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    const float gs = 2.0f * inv_n * gloss[0];
    const size_t vs = (size_t)Cout * HW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        const float4 nh = *reinterpret_cast<const float4*>(noise_hat + o);
        const float4 t = *reinterpret_cast<const float4*>(target + o);
        const float4 g = make_float4(gs * (nh.x - t.x), gs * (nh.y - t.y), gs * (nh.z - t.z), gs * (nh.w - t.w));
        if (!weighting) {
            const float inv = 1.0f / (float)(v1 - v0);
            const float4 d = make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv);
            for (int v = v0; v < v1; ++v) {
                *reinterpret_cast<float4*>(dout + (size_t)v * vs + (size_t)c * HW + p) = d;
                if (Cout > 3)
                    *reinterpret_cast<float4*>(dout + (size_t)v * vs + (size_t)(3 + c) * HW + p) =
                        make_float4(0.f, 0.f, 0.f, 0.f);
            }
            continue;
        }
        float4 mx, inv;
        (void)compose4(out, Cout, HW, v0, v1, c, p, 1, &mx, &inv);
        for (int v = v0; v < v1; ++v) {
            const float* ep = out + (size_t)v * vs + (size_t)c * HW + p;
            const float4 e = *reinterpret_cast<const float4*>(ep);
            const float4 l = *reinterpret_cast<const float4*>(ep + (size_t)3 * HW);
            const float4 w = make_float4(expf(l.x - mx.x) * inv.x, expf(l.y - mx.y) * inv.y, expf(l.z - mx.z) * inv.z,
                                         expf(l.w - mx.w) * inv.w);
            float* dp = dout + (size_t)v * vs + (size_t)c * HW + p;
            *reinterpret_cast<float4*>(dp) = make_float4(w.x * g.x, w.y * g.y, w.z * g.z, w.w * g.w);
            *reinterpret_cast<float4*>(dp + (size_t)3 * HW) =
                make_float4(w.x * (e.x - nh.x) * g.x, w.y * (e.y - nh.y) * g.y, w.z * (e.z - nh.z) * g.z,
                            w.w * (e.w - nh.w) * g.w);
        }
    }
}

// y0_hat of one element, as the composing tails write it.  How it is rounded there is the compiler's choice per body
// (held fixed by the instruction-stream comparison of profiles/threshold.md): the ancestral tails round b eps and fuse the
// rest, fma(a, y, -(b eps)); the few-step tails round both products and subtract.  The tails on the eps buffer and the
// statistics kernel say explicitly which (FUSED), so that a sample whose threshold is 1 gets the static clamp's bits and
// the selection sees exactly the values the tail bounds.
__device__ __forceinline__ float y0_hat(float a, float y, float b, float eps) { return a * y - b * eps; }
// (Pinned arithmetic: contraction is off inside these functions, so a product or a sum written here is rounded as
// written, and a fused multiply-add is one only where __builtin_fmaf says so.)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
template <bool FUSED>
__device__ __forceinline__ float y0_hat_as(float a, float y, float b, float eps) {
    if constexpr (FUSED) return __builtin_fmaf(a, y, -mul_rn(b, eps));
    return add_rn(mul_rn(a, y), -mul_rn(b, eps));
}

// y0 -> y_next, the one copy of each flavour's update.  PINNED = false is the expression the composing tails have always
// compiled; PINNED = true (the tails on the eps buffer) writes out, operation by operation, the roundings the compiler
// gives that expression in ALL of those tails (read off their instruction stream, which the comparison of
// profiles/threshold.md holds fixed), so that a sample whose threshold is 1 gets the static clamp's bits:
//   ancestral: mean = fma(c2, y, c1 y0), y_next = fma(z, sd, mean), every element;
//   few-step:  cy y + c0 y0 is fma(cy, y, c0 y0) in elements 0, 1 of a float4 and both products rounded, then added, in
//              elements 2, 3 (the packed-math schedule of that body); the history and noise terms are fused onto it.
template <bool PINNED>
__device__ __forceinline__ void posterior_update(float c1, float c2, float sd, float y0, float y, float z, float& m,
                                                 float& r) {
    if constexpr (PINNED) {
        m = __builtin_fmaf(c2, y, mul_rn(c1, y0));
        r = __builtin_fmaf(z, sd, m);
    } else {
        m = c1 * y0 + c2 * y;
        r = m + z * sd;
    }
}
template <bool PINNED>
__device__ __forceinline__ float multistep_base(float cy, float y, float c0, float y0, int j) {
    if constexpr (PINNED)
        return j < 2 ? __builtin_fmaf(cy, y, mul_rn(c0, y0)) : add_rn(mul_rn(cy, y), mul_rn(c0, y0));
    return cy * y + c0 * y0;
}
template <bool PINNED>
__device__ __forceinline__ float multistep_add(float r, float c, float v) {
    if constexpr (PINNED) return __builtin_fmaf(c, v, r);
    return r + c * v;
}

// What the tails that read the composed-eps buffer know about their sample (the head of this file holds the definition):
// stat[b] = {r_b, s_b} from sample_stat_kernel.  rescale == 0: eps is the buffer's value, no multiply; thr == 0: the
// static clamp under `clip`, as in the composing tails.
struct EpsBound {
    float r, s;
    int thr;
    __device__ __forceinline__ float operator()(float v, int clip) const {
        if (thr) return fminf(fmaxf(v, -s), s) / s;
        return clip ? fminf(fmaxf(v, -1.0f), 1.0f) : v;
    }
};
struct EpsBuffer {
    const float* __restrict__ eps = nullptr;      // eps_g [B][3][HW]
    const float2* __restrict__ stat = nullptr;    // [B]
    int rescale = 0, thr = 0;
    __device__ __forceinline__ EpsBound bound(int b) const {
        EpsBound l{1.0f, 1.0f, thr};
        if (stat != nullptr && (rescale || thr)) {
            const float2 st = stat[b];
            l.r = st.x;
            l.s = st.y;
        }
        return l;
    }
    __device__ __forceinline__ float4 load(size_t o, const EpsBound& l) const {
        float4 e = *reinterpret_cast<const float4*>(eps + o);
        if (rescale) e = make_float4(l.r * e.x, l.r * e.y, l.r * e.z, l.r * e.w);
        return e;
    }
};

// ---- the reverse-step tails: two kernel templates, three switches each ----
//   CFG: `out` has off[B] + B rows and the composed eps is guided by the sample's null row with the scale gscale[b].
//   EPS (the source of eps, implies !CFG): false -- composed (+ guided) here from `out`, static clamp, weights written;
//        true -- read back from the composed-eps pass (eps_buf, stat, rescale, thr: EpsBuffer above; dynamic threshold),
//        and `out`, `off`, `weights`, `gscale`, Cout, maxV and weighting are not touched.
//   RNG: false -- z is loaded (z == null: no noise); true -- z is drawn here from (seed, ids[b], step, float4 index).
// Every instantiation has the one argument list; what its switches do not use is dead (the launchers pass null / 0).
// t / kidx / ids / stat live in device memory, so a captured launch replays for every step.  grid (chunks, B).

// The two noise sources, each defined here and nowhere else: noise(i, o) gives z for float4 i of the sample
// (o = its float offset in [B][3][HW]).  Loaded: z[o], and no buffer is no noise.  Drawn: Philox, kind 3, block = the
// float4 index, keyed by the sample's id and the tail's `step`; ZERO_AT_0 (the ancestral chain): z = 0 where step == 0.
__device__ __forceinline__ auto load_z(const float* z) {
    return [z](int, size_t o) {
        float4 zz = make_float4(0.f, 0.f, 0.f, 0.f);
        if (z) zz = *reinterpret_cast<const float4*>(z + o);
        return zz;
    };
}
template <bool ZERO_AT_0>
__device__ __forceinline__ auto draw_z(unsigned long long seed, unsigned long long id, long long step) {
    return [seed, id, step](int i, size_t) {
        float n[4] = {0.f, 0.f, 0.f, 0.f};
        if (!ZERO_AT_0 || step != 0) vf_rng_normal4(seed, id, VF_RNG_STEP_NOISE, (uint32_t)step, (uint32_t)i, n);
        return make_float4(n[0], n[1], n[2], n[3]);
    };
}
template <bool RNG, bool ZERO_AT_0>
__device__ __forceinline__ auto tail_noise(const float* z, unsigned long long seed, const long long* ids,
                                           long long step) {
    if constexpr (RNG) return draw_z<ZERO_AT_0>(seed, (unsigned long long)ids[blockIdx.y], step);
    else return load_z(z);
}

// The common prologue of the two tails.  What a workgroup knows about its sample b = blockIdx.y before the element loop:
// its rows [v0, v1) of `out`, its guidance scale g (gm = 1 - g) and null row eu, its rescale and threshold lim ...
struct TailSample {
    int v0 = 0, v1 = 0;
    float g = 1.0f, gm = 0.0f;
    const float* eu = nullptr;
    EpsBound lim;
};
template <bool CFG, bool EPS>
__device__ __forceinline__ TailSample tail_sample(const float* __restrict__ out, const int* __restrict__ off,
                                                  const float* __restrict__ gscale, const EpsBuffer& src, int Cout,
                                                  int HW) {
    const int b = blockIdx.y;
    TailSample s;
    if constexpr (!EPS) {
        s.v0 = off[b];
        s.v1 = off[b + 1];
    }
    if constexpr (CFG) {
        s.g = gscale[b];
        s.gm = 1.0f - s.g;
        s.eu = out + (size_t)(off[gridDim.y] + b) * Cout * HW;
    }
    s.lim = src.bound(b);
    return s;
}
// ... and the eps of its float4 (c, p) at float offset o: compose -> guide, or the load from the eps buffer.
template <bool CFG, bool EPS>
__device__ __forceinline__ float4 tail_eps(const TailSample& s, const float* __restrict__ out, const EpsBuffer& src,
                                           int Cout, int HW, int weighting, int c, int p, size_t o, float4* mx,
                                           float4* inv) {
    if constexpr (EPS) {
        return src.load(o, s.lim);
    } else {
        float4 eps = compose4(out, Cout, HW, s.v0, s.v1, c, p, weighting, mx, inv);
        if constexpr (CFG) eps = guide4(eps, s.eu + (size_t)c * HW + p, s.g, s.gm);
        return eps;
    }
}

// One reverse step after the UNet: compose -> y0_hat = a_t y_t - b_t eps -> clamp ->
// mean = c1 y0_hat + c2 y_t -> y_{t-1} = mean + z * exp(0.5 logvar).
// RNG: step = t[b], and z = 0 where t[b] == 0.  Everything from y0 on is shared by all six instantiations.
template <bool CFG, bool EPS, bool RNG>
__global__ __launch_bounds__(256) void p_sample_tail_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ eps_buf,
    const float2* __restrict__ stat, const float* __restrict__ y_t, const float* __restrict__ z,
    unsigned long long seed, const long long* __restrict__ ids, const long long* __restrict__ t,
    const float* __restrict__ sqrt_recip, const float* __restrict__ sqrt_recipm1, const float* __restrict__ logvar,
    const float* __restrict__ coef1, const float* __restrict__ coef2, float* __restrict__ y_next,
    float* __restrict__ mean_out, float* __restrict__ weights, int Cout, int HW, int maxV, int weighting, int clip,
    const float* __restrict__ gscale, int rescale, int thr) {
    static_assert(!(CFG && EPS), "guidance happens in the composed-eps pass");
    const int b = blockIdx.y;
    const EpsBuffer src{eps_buf, stat, rescale, thr};
    const TailSample s = tail_sample<CFG, EPS>(out, off, gscale, src, Cout, HW);
    const int n4 = 3 * HW / 4;
    const long long tb = t[b];
    const auto noise = tail_noise<RNG, true>(z, seed, ids, tb);
    const float a_t = sqrt_recip[tb], b_t = sqrt_recipm1[tb], c1 = coef1[tb], c2 = coef2[tb];
    const float sd = expf(0.5f * logvar[tb]);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        float4 mx, inv;
        const float4 eps = tail_eps<CFG, EPS>(s, out, src, Cout, HW, weighting, c, p, o, &mx, &inv);
        const float4 y = *reinterpret_cast<const float4*>(y_t + o);
        float y0[4] = {y0_hat(a_t, y.x, b_t, eps.x), y0_hat(a_t, y.y, b_t, eps.y), y0_hat(a_t, y.z, b_t, eps.z),
                       y0_hat(a_t, y.w, b_t, eps.w)};
        if constexpr (EPS) {
            y0[0] = y0_hat_as<true>(a_t, y.x, b_t, eps.x);
            y0[1] = y0_hat_as<true>(a_t, y.y, b_t, eps.y);
            y0[2] = y0_hat_as<true>(a_t, y.z, b_t, eps.z);
            y0[3] = y0_hat_as<true>(a_t, y.w, b_t, eps.w);
        }
        const float ys[4] = {y.x, y.y, y.z, y.w};
        float m[4], r[4];
        const float4 zz = noise(i, o);
        const float zs[4] = {zz.x, zz.y, zz.z, zz.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (EPS) y0[k] = s.lim(y0[k], clip);
            else if (clip) y0[k] = fminf(fmaxf(y0[k], -1.0f), 1.0f);
            posterior_update<EPS>(c1, c2, sd, y0[k], ys[k], zs[k], m[k], r[k]);
        }
        if (y_next) *reinterpret_cast<float4*>(y_next + o) = make_float4(r[0], r[1], r[2], r[3]);
        if (mean_out) *reinterpret_cast<float4*>(mean_out + o) = make_float4(m[0], m[1], m[2], m[3]);
        if constexpr (!EPS)
            if (weights && weighting) write_weights(out, weights, Cout, HW, maxV, s.v0, s.v1, c, p, i, mx, inv);
    }
}

// One linear-multistep reverse step after the UNet (strided DDIM, DPM-Solver++ 2M; schedule.sampler_tables):
//   y0 = clamp(a[k] y - b[k] eps, -1, 1);  y_new = cy[k] y + c0[k] y0 + c1[k] y0_prev + sigma[k] z;  y0_prev <- y0
// with k = kidx[b] read from device memory.  sigma[k] == 0: `noise` is never called (no load, no draw);
// c1[k] == 0 or no history buffer: y0_prev is not read (it may hold anything before the first multistep step).
// Elementwise: y_next may be y, and y0_prev is read and written by the same thread.
// RNG: step = the MODEL timestep tau[k], so a strided chain and the full chain draw the same z at the same noise level.
template <bool CFG, bool EPS, bool RNG>
__global__ __launch_bounds__(256) void sampler_step_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ eps_buf,
    const float2* __restrict__ stat, const float* __restrict__ y_t, const float* __restrict__ z,
    unsigned long long seed, const long long* __restrict__ ids, const long long* __restrict__ kidx,
    const long long* __restrict__ tau, const float* __restrict__ ta, const float* __restrict__ tb,
    const float* __restrict__ tcy, const float* __restrict__ tc0, const float* __restrict__ tc1,
    const float* __restrict__ tsigma, float* y0_prev, float* __restrict__ y_next, float* __restrict__ weights, int Cout,
    int HW, int maxV, int weighting, const float* __restrict__ gscale, int rescale, int thr) {
    static_assert(!(CFG && EPS), "guidance happens in the composed-eps pass");
    const int b = blockIdx.y;
    const EpsBuffer src{eps_buf, stat, rescale, thr};
    const TailSample s = tail_sample<CFG, EPS>(out, off, gscale, src, Cout, HW);
    const int n4 = 3 * HW / 4;
    const long long k = kidx[b];
    const auto noise = tail_noise<RNG, false>(z, seed, ids, RNG ? (uint32_t)tau[k] : 0u);
    const float a_k = ta[k], b_k = tb[k], cy = tcy[k], c0 = tc0[k], c1 = tc1[k], sg = tsigma[k];
    const bool hist = y0_prev != nullptr && c1 != 0.0f, noisy = sg != 0.0f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        float4 mx, inv;
        const float4 eps = tail_eps<CFG, EPS>(s, out, src, Cout, HW, weighting, c, p, o, &mx, &inv);
        const float4 y = *reinterpret_cast<const float4*>(y_t + o);
        const float ys[4] = {y.x, y.y, y.z, y.w};
        const float es[4] = {eps.x, eps.y, eps.z, eps.w};
        float y0[4], r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (EPS) y0[j] = s.lim(y0_hat_as<false>(a_k, ys[j], b_k, es[j]), 1);
            else y0[j] = fminf(fmaxf(y0_hat(a_k, ys[j], b_k, es[j]), -1.0f), 1.0f);
            r[j] = multistep_base<EPS>(cy, ys[j], c0, y0[j], j);
        }
        if (hist) {
            const float4 h = *reinterpret_cast<const float4*>(y0_prev + o);
            r[0] = multistep_add<EPS>(r[0], c1, h.x); r[1] = multistep_add<EPS>(r[1], c1, h.y);
            r[2] = multistep_add<EPS>(r[2], c1, h.z); r[3] = multistep_add<EPS>(r[3], c1, h.w);
        }
        if (noisy) {
            const float4 zz = noise(i, o);
            r[0] = multistep_add<EPS>(r[0], sg, zz.x); r[1] = multistep_add<EPS>(r[1], sg, zz.y);
            r[2] = multistep_add<EPS>(r[2], sg, zz.z); r[3] = multistep_add<EPS>(r[3], sg, zz.w);
        }
        if (y0_prev) *reinterpret_cast<float4*>(y0_prev + o) = make_float4(y0[0], y0[1], y0[2], y0[3]);
        *reinterpret_cast<float4*>(y_next + o) = make_float4(r[0], r[1], r[2], r[3]);
        if constexpr (!EPS)
            if (weights && weighting) write_weights(out, weights, Cout, HW, maxV, s.v0, s.v1, c, p, i, mx, inv);
    }
}

// Training draws of sample b (kind 0): t[b] in [1, T-1] as int64, u[b] in [0, 1) (optional output) and
// level[b] = (g[t] - g[t-1]) u + g[t-1]  (view_fusion.py:229-237).
__global__ void draw_train_kernel(unsigned long long seed, const long long* __restrict__ ids,
                                  const float* __restrict__ gammas, int T, long long* __restrict__ t,
                                  float* __restrict__ u, float* __restrict__ level, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t w[4];
    vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
    const long long tb = vf_rng_timestep(w[0], T);
    const float ub = vf_rng_uniform24(w[1]);
    const float hi = gammas[tb], lo = gammas[tb - 1];
    t[b] = tb;
    if (u) u[b] = ub;
    level[b] = (hi - lo) * ub + lo;
}

// out[b][4 i .. 4 i + 3] = the four normals of (seed, ids[b], kind, step, block i); grid (chunks, B)
__global__ __launch_bounds__(256) void randn_ids_kernel(unsigned long long seed, const long long* __restrict__ ids,
                                                        int kind, int step, float4* __restrict__ out, int n4) {
    const unsigned long long id = (unsigned long long)ids[blockIdx.y];
    float4* o = out + (size_t)blockIdx.y * n4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        float n[4];
        vf_rng_normal4(seed, id, (uint32_t)kind, (uint32_t)step, (uint32_t)i, n);
        o[i] = make_float4(n[0], n[1], n[2], n[3]);
    }
}

// the raw words of the same counters (tests: device against host)
__global__ __launch_bounds__(256) void philox_ids_kernel(unsigned long long seed, const long long* __restrict__ ids,
                                                         int kind, int step, uint4* __restrict__ out, int n4) {
    const unsigned long long id = (unsigned long long)ids[blockIdx.y];
    uint4* o = out + (size_t)blockIdx.y * n4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        uint32_t w[4];
        vf_rng_words(seed, id, (uint32_t)kind, (uint32_t)step, (uint32_t)i, w);
        o[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// level[b] = table[t[b]]  (extract(), view_fusion.py:314-317) or the training draw
// level = (g[t]-g[t-1])*u + g[t-1]  (view_fusion.py:231-237) when u != null.
__global__ void gather_level_kernel(const float* __restrict__ gammas, const long long* __restrict__ t,
                                    const float* __restrict__ u, float* __restrict__ level, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const long long tb = t[b];
    const float hi = gammas[tb];
    if (u) {
        const float lo = gammas[tb - 1];
        level[b] = (hi - lo) * u[b] + lo;
    } else {
        level[b] = hi;
    }
}

// psnr[b] = 20 log10(1 / sqrt(mean((a-b)^2)))  -- one workgroup per image (utils/metrics.py:6-8)
__global__ __launch_bounds__(256) void psnr_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                   float* __restrict__ out, int n) {
    __shared__ float red[4];
    const float4* a4 = reinterpret_cast<const float4*>(a + (size_t)blockIdx.x * n);
    const float4* b4 = reinterpret_cast<const float4*>(b + (size_t)blockIdx.x * n);
    float s = 0.f;
    for (int i = threadIdx.x; i < (n >> 2); i += 256) {
        const float4 u = a4[i], v = b4[i];
        const float dx = u.x - v.x, dy = u.y - v.y, dz = u.z - v.z, dw = u.w - v.w;
        s += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = 20.0f * log10f(1.0f / sqrtf(s / (float)n));
}

// ---- the loss family: penalty x prediction x noise-level weight, per-sample loss and scale, loss-by-level histogram
// (loss_weight.h, level_sampler.h; the head of this file holds the table of targets) ----
// The training target of one element:
//   eps the ready-made target handed over as `noise` (y_0 and level are not read);
//   v   sa noise - sb y_0 with sa = sqrtf(g_b), sb = sqrtf(1 - g_b), formed in registers from the noise and y_0 the step
//       already holds: sb y_0 is rounded, the rest is one fused multiply-add, written out so that the forward and the
//       backward kernel form the very same bits;
//   x0  y_0 itself (the noise is not read).
template <int PRED>
__device__ __forceinline__ float4 pred_target4(const float* __restrict__ noise, const float* __restrict__ y_0, size_t o,
                                               float sa, float sb) {
    if (PRED == VF_PRED_EPS) return *reinterpret_cast<const float4*>(noise + o);
    const float4 y = *reinterpret_cast<const float4*>(y_0 + o);
    if (PRED == VF_PRED_X0) return y;
    const float4 n = *reinterpret_cast<const float4*>(noise + o);
    return make_float4(__builtin_fmaf(sa, n.x, -mul_rn(sb, y.x)), __builtin_fmaf(sa, n.y, -mul_rn(sb, y.y)),
                       __builtin_fmaf(sa, n.z, -mul_rn(sb, y.z)), __builtin_fmaf(sa, n.w, -mul_rn(sb, y.w)));
}

// ---- learned variance inside the family (the head of this file holds the definition, vlb.h the arithmetic) ----
// o_b of one float4 (c, p): channel 6 + c composed under the weights of channel c -- the softmax of channel 3 + c with
// the (mx, inv) compose4 handed back, or the mean.
__device__ __forceinline__ float4 compose4_var(const float* __restrict__ out, int Cout, int HW, int v0, int v1, int c,
                                               int p, int weighting, const float4& mx, const float4& inv) {
    const size_t vs = (size_t)Cout * HW;
    const float* l0 = out + (size_t)v0 * vs + (size_t)(3 + c) * HW + p;
    const float* o0 = l0 + (size_t)3 * HW;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!weighting) {
        for (int v = v0; v < v1; ++v) {
            const float4 o = *reinterpret_cast<const float4*>(o0 + (size_t)(v - v0) * vs);
            acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
        }
        const float n = 1.0f / (float)(v1 - v0);
        return make_float4(acc.x * n, acc.y * n, acc.z * n, acc.w * n);
    }
    for (int v = v0; v < v1; ++v) {
        const float4 l = *reinterpret_cast<const float4*>(l0 + (size_t)(v - v0) * vs);
        const float4 o = *reinterpret_cast<const float4*>(o0 + (size_t)(v - v0) * vs);
        acc.x += expf(l.x - mx.x) * o.x; acc.y += expf(l.y - mx.y) * o.y;
        acc.z += expf(l.z - mx.z) * o.z; acc.w += expf(l.w - mx.w) * o.w;
    }
    return make_float4(acc.x * inv.x, acc.y * inv.y, acc.z * inv.z, acc.w * inv.w);
}

// What only the LV instantiations read, handed over by value behind the family's own operands: t (int64 [B]), the fp32
// tables c1, hi, lo [T] and the weight of the vlb term.  The others take it empty and do not look at it.
struct VlbArgs {
    const long long* t;
    const float *c1, *hi, *lo;
    int T;
    float lambda;
};

// The operands of the three kernels that exist with LV alone, by value at the END of the argument list.  Without LV the
// struct is empty: the argument list, and so the code, of those instantiations is what it was before the switch existed
// (a run-time null check in the finish kernel and 56 / 48 unused kernarg bytes in the other two were measured: the non-LV
// forward + backward pairs came out 1 - 1.7 % slower; profiles/loss_lv_templates.md).
template <bool LV> struct VlbFwd {};
template <> struct VlbFwd<true> { VlbArgs vlb; float* var_hat; float* vlb_part; };
template <bool LV> struct VlbBwd {};
template <> struct VlbBwd<true> { VlbArgs vlb; const float* var_hat; };
template <bool LV> struct VlbFinish {};
template <> struct VlbFinish<true> { const float* vlb_part; float* sample_vlb; float lambda; };

// What a workgroup of the hybrid loss knows about its sample: the tables at t[b] (clamped into [0, T - 1] before any
// table is read) and kappa^2 of its level.
struct VlbSample {
    float c1, hi, lo, k2;
};
template <int PRED>
__device__ __forceinline__ VlbSample vlb_sample(const VlbArgs& a, float g) {
    long long tb = a.t[blockIdx.y];
    tb = tb < 0 ? 0 : (tb > a.T - 1 ? a.T - 1 : tb);
    return VlbSample{a.c1[tb], a.hi[tb], a.lo[tb], vf_vlb_kappa2(PRED, g)};
}

// compose_fwd_kernel with a penalty and a prediction: the same composition and the same (b, chunk) partial sums, of
// rho(noise_hat - target).  noise_hat receives the composed output in the network's own parameterisation (what the
// backward kernel reads back).  LV: plus the variance channels -- next to those partial sums the partial sums of
// KL(r, o_b) in bits, on the same residual r, and var_hat receives the composed o_b.
template <int PEN, int PRED, bool LV>
__global__ __launch_bounds__(256) void compose_loss_fwd_kernel(const float* __restrict__ out,
                                                               const int* __restrict__ off,
                                                               const float* __restrict__ noise,
                                                               const float* __restrict__ y_0,
                                                               const float* __restrict__ level,
                                                               float* __restrict__ noise_hat,
                                                               float* __restrict__ loss_part, int Cout, int HW,
                                                               int weighting, float delta, VlbFwd<LV> vo) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    float g = 0.f, sa = 0.f, sb = 0.f;
    if (LV || PRED != VF_PRED_EPS) g = level[b];
    if (PRED != VF_PRED_EPS) sa = sqrtf(g), sb = sqrtf(1.0f - g);
    VlbSample s{};
    if constexpr (LV) s = vlb_sample<PRED>(vo.vlb, g);
    float acc = 0.f, kl = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        float4 mx = make_float4(0.f, 0.f, 0.f, 0.f), inv = mx, ob = mx;
        const float4 nh = compose4(out, Cout, HW, v0, v1, c, p, weighting, LV ? &mx : nullptr, LV ? &inv : nullptr);
        if constexpr (LV) ob = compose4_var(out, Cout, HW, v0, v1, c, p, weighting, mx, inv);
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        *reinterpret_cast<float4*>(noise_hat + o) = nh;
        if constexpr (LV) *reinterpret_cast<float4*>(vo.var_hat + o) = ob;
        const float4 t = pred_target4<PRED>(noise, y_0, o, sa, sb);
        const float r[4] = {nh.x - t.x, nh.y - t.y, nh.z - t.z, nh.w - t.w};
        acc += (vf_loss_rho<PEN>(r[0], delta) + vf_loss_rho<PEN>(r[1], delta)) +
               (vf_loss_rho<PEN>(r[2], delta) + vf_loss_rho<PEN>(r[3], delta));
        if constexpr (LV) {
            const float os[4] = {ob.x, ob.y, ob.z, ob.w};
            float k[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                k[j] = vf_vlb_kl(vf_vlb_logvar(os[j], s.hi, s.lo), s.lo, vf_vlb_m2(s.c1, s.k2, r[j]));
            kl += (k[0] + k[1]) + (k[2] + k[3]);
        }
    }
    acc = block_sum<256>(acc, red);
    if constexpr (LV) kl = block_sum<256>(kl, red);
    if (threadIdx.x == 0) {
        loss_part[blockIdx.y * gridDim.x + blockIdx.x] = acc;
        if constexpr (LV) vo.vlb_part[blockIdx.y * gridDim.x + blockIdx.x] = kl;
    }
}

// One workgroup.  Per sample (one thread each): s_b = its `ch` partials in index order / n, w_b = the native weight of
// its level for the prediction (vf_loss_weight_pred; pred 0 is vf_loss_weight); then loss = sum_b sample_w[b] s_b / B in
// index order (one thread); then, with a histogram attached, one thread per bin walks the samples in index order and adds
// the UNWEIGHTED s_b of its own bin into the persistent accumulators.  scale (nullable; the importance weight of a
// level-sampler draw): with it sample_w holds 2 B floats -- w_s scale[s], what the loss and the backward kernel use, then
// w_s alone, what level_stats_kernel reads; without, B floats.  LV (vlb_part, sample_vlb and lambda in `vo`; never
// with scale: a level sampler is refused with a learned variance): sample_vlb[s] = its `ch` partials in index order / n,
// and loss = sum_s sample_w[s] sample_loss[s] / B + lambda sum_s sample_vlb[s] / B, each sum in index order by one
// thread; the histogram stays L_simple's alone.  Every address is written by exactly one thread: no atomics, the same
// bits on every run.
template <bool LV>
__global__ __launch_bounds__(64) void compose_loss_finish_kernel(const float* __restrict__ part,
                                                                 const float* __restrict__ level,
                                                                 const float* __restrict__ scale,
                                                                 float* __restrict__ sample_loss,
                                                                 float* __restrict__ sample_w, float* __restrict__ loss,
                                                                 float* __restrict__ bin_sum, int* __restrict__ bin_cnt,
                                                                 int B, int ch, int K, float inv_n, int kind, float a,
                                                                 float b, int pred, VlbFinish<LV> vo) {
    for (int s = threadIdx.x; s < B; s += 64) {
        float acc = 0.f;
        for (int c = 0; c < ch; ++c) acc += part[s * ch + c];
        sample_loss[s] = acc * inv_n;
        if constexpr (LV) {
            float kl = 0.f;
            for (int c = 0; c < ch; ++c) kl += vo.vlb_part[s * ch + c];
            vo.sample_vlb[s] = kl * inv_n;
        }
        const float w = vf_loss_weight_pred(pred, kind, a, b, level[s]);
        if (!LV && scale != nullptr) {      // (never both: the LV instantiation holds no scale path)
            sample_w[s] = w * scale[s];
            sample_w[B + s] = w;
        } else {
            sample_w[s] = w;
        }
    }
    __syncthreads();                        // (also makes the workgroup's global stores above visible to it)
    if (threadIdx.x == 0) {
        float acc = 0.f;
        for (int s = 0; s < B; ++s) acc += sample_w[s] * sample_loss[s];
        if constexpr (LV) {
            float kl = 0.f;
            for (int s = 0; s < B; ++s) kl += vo.sample_vlb[s];
            *loss = acc / (float)B + vo.lambda * (kl / (float)B);
        } else {
            *loss = acc / (float)B;
        }
    }
    if (bin_sum == nullptr) return;
    for (int k = threadIdx.x; k < K; k += 64) {
        float sum = 0.f;
        int cnt = 0;
        for (int s = 0; s < B; ++s) {
            int bin = (int)(level[s] * (float)K);
            bin = bin > K - 1 ? K - 1 : bin;
            if (bin == k) {
                sum += sample_loss[s];
                ++cnt;
            }
        }
        bin_sum[k] += sum;
        bin_cnt[k] += cnt;
    }
}

// compose_mse_bwd_kernel with a penalty and a prediction: the forward kernel's target formed again, g = gloss
// sample_w[b] rho'(noise_hat - target) / (n B), then the same softmax / mean chain rule (d eps_v = w_v g;
// d logit_v = w_v (eps_v - nh) g;  mean ablation: d eps_v = g / count, logits zero).
// LV: into nine channels.  g stays L_simple's gradient on the composed prediction; gv = gloss lambda / (n B) dKL/dlp
// 0.5 (hi - lo) is the vlb term's gradient on o_b, with the residual a constant.  Then
//   channels 0..2  w_v g                                     (mean: g / count)
//   channels 3..5  w_v (e_v - nh) g + w_v (o_v - o_b) gv     (mean: 0)
//   channels 6..8  w_v gv                                    (mean: gv / count)
// every address of dout's nine channels written exactly once.
template <int PEN, int PRED, bool LV>
__global__ __launch_bounds__(256) void compose_loss_bwd_kernel(const float* __restrict__ out,
                                                               const int* __restrict__ off,
                                                               const float* __restrict__ noise,
                                                               const float* __restrict__ y_0,
                                                               const float* __restrict__ level,
                                                               const float* __restrict__ noise_hat,
                                                               const float* __restrict__ gloss,
                                                               const float* __restrict__ sample_w,
                                                               float* __restrict__ dout, int Cout, int HW,
                                                               int weighting, float inv_nb, float delta, VlbBwd<LV> vo) {
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    const float gs = gloss[0] * sample_w[b] * inv_nb;
    float g_b = 0.f, sa = 0.f, sb = 0.f;
    if (LV || PRED != VF_PRED_EPS) g_b = level[b];
    if (PRED != VF_PRED_EPS) sa = sqrtf(g_b), sb = sqrtf(1.0f - g_b);
    VlbSample s{};
    float gvs = 0.f;
    if constexpr (LV) {
        s = vlb_sample<PRED>(vo.vlb, g_b);
        gvs = gloss[0] * vo.vlb.lambda * inv_nb * (0.5f * (s.hi - s.lo));
    }
    const size_t vs = (size_t)Cout * HW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        const float4 nh = *reinterpret_cast<const float4*>(noise_hat + o);
        float4 ob = make_float4(0.f, 0.f, 0.f, 0.f), gv = ob;
        if constexpr (LV) ob = *reinterpret_cast<const float4*>(vo.var_hat + o);
        const float4 t = pred_target4<PRED>(noise, y_0, o, sa, sb);
        const float r[4] = {nh.x - t.x, nh.y - t.y, nh.z - t.z, nh.w - t.w};
        const float4 g = make_float4(gs * vf_loss_drho<PEN>(r[0], delta), gs * vf_loss_drho<PEN>(r[1], delta),
                                     gs * vf_loss_drho<PEN>(r[2], delta), gs * vf_loss_drho<PEN>(r[3], delta));
        if constexpr (LV) {
            const float os[4] = {ob.x, ob.y, ob.z, ob.w};
            float gk[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                gk[j] = gvs * vf_vlb_dkl(vf_vlb_logvar(os[j], s.hi, s.lo), s.lo, vf_vlb_m2(s.c1, s.k2, r[j]));
            gv = make_float4(gk[0], gk[1], gk[2], gk[3]);
        }
        if (!weighting) {
            const float inv = 1.0f / (float)(v1 - v0);
            const float4 d = make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv);
            const float4 dv = make_float4(gv.x * inv, gv.y * inv, gv.z * inv, gv.w * inv);
            for (int v = v0; v < v1; ++v) {
                if constexpr (LV) {
                    float* dp = dout + (size_t)v * vs + (size_t)c * HW + p;
                    *reinterpret_cast<float4*>(dp) = d;
                    *reinterpret_cast<float4*>(dp + (size_t)3 * HW) = make_float4(0.f, 0.f, 0.f, 0.f);
                    *reinterpret_cast<float4*>(dp + (size_t)6 * HW) = dv;
                } else {            // (written out: behind a shared base pointer these instantiations' code changes)
                    *reinterpret_cast<float4*>(dout + (size_t)v * vs + (size_t)c * HW + p) = d;
                    if (Cout > 3)
                        *reinterpret_cast<float4*>(dout + (size_t)v * vs + (size_t)(3 + c) * HW + p) =
                            make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            continue;
        }
        float4 mx, inv;
        (void)compose4(out, Cout, HW, v0, v1, c, p, 1, &mx, &inv);
        for (int v = v0; v < v1; ++v) {
            const float* ep = out + (size_t)v * vs + (size_t)c * HW + p;
            const float4 e = *reinterpret_cast<const float4*>(ep);
            const float4 l = *reinterpret_cast<const float4*>(ep + (size_t)3 * HW);
            const float4 w = make_float4(expf(l.x - mx.x) * inv.x, expf(l.y - mx.y) * inv.y, expf(l.z - mx.z) * inv.z,
                                         expf(l.w - mx.w) * inv.w);
            float* dp = dout + (size_t)v * vs + (size_t)c * HW + p;
            *reinterpret_cast<float4*>(dp) = make_float4(w.x * g.x, w.y * g.y, w.z * g.z, w.w * g.w);
            if constexpr (LV) {
                const float4 q = *reinterpret_cast<const float4*>(ep + (size_t)6 * HW);
                *reinterpret_cast<float4*>(dp + (size_t)3 * HW) =
                    make_float4(w.x * (e.x - nh.x) * g.x + w.x * (q.x - ob.x) * gv.x,
                                w.y * (e.y - nh.y) * g.y + w.y * (q.y - ob.y) * gv.y,
                                w.z * (e.z - nh.z) * g.z + w.z * (q.z - ob.z) * gv.z,
                                w.w * (e.w - nh.w) * g.w + w.w * (q.w - ob.w) * gv.w);
                *reinterpret_cast<float4*>(dp + (size_t)6 * HW) = make_float4(w.x * gv.x, w.y * gv.y, w.z * gv.z, w.w * gv.w);
            } else {
                *reinterpret_cast<float4*>(dp + (size_t)3 * HW) =
                    make_float4(w.x * (e.x - nh.x) * g.x, w.y * (e.y - nh.y) * g.y, w.z * (e.z - nh.z) * g.z,
                                w.w * (e.w - nh.w) * g.w);
            }
        }
    }
}

// ---- loss-aware noise-level sampling (level_sampler.h holds the specification) ----
// draw_train_kernel's sibling: t from the proposal table (c [K + 1], iw [K], *ready in device memory) instead of the
// uniform map, and the draw's importance weight.  The word is word 0 of the sample's training-scalars call (ids != null)
// or words[b] (the unseeded path: int64 values in [0, 2^32)); u / level (seeded only, both optional) as draw_train_kernel.
__global__ void draw_level_kernel(unsigned long long seed, const long long* __restrict__ ids,
                                  const long long* __restrict__ words, const float* __restrict__ gammas, int T, int K,
                                  const unsigned long long* __restrict__ c, const float* __restrict__ iw,
                                  const int* __restrict__ ready, long long* __restrict__ t, float* __restrict__ u,
                                  float* __restrict__ level, float* __restrict__ iw_out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (ids) vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
    else w[0] = (uint32_t)words[b];
    long long tb;
    float wb = 1.0f;
    if (*ready) {
        int k;
        tb = vf_level_draw(w[0], c, T, K, &k);
        tb = tb < 1 ? 1 : (tb > T - 1 ? T - 1 : tb);     // (a table that breaks its invariants must not index past gammas)
        wb = iw[k];
    } else {
        tb = vf_rng_timestep(w[0], T);
    }
    t[b] = tb;
    iw_out[b] = wb;
    if (ids == nullptr) return;
    const float ub = vf_rng_uniform24(w[1]);
    if (u) u[b] = ub;
    if (level) {
        const float hi = gammas[tb], lo = gammas[tb - 1];
        level[b] = (hi - lo) * ub + lo;
    }
}

// One workgroup of 256 threads.  One thread per bin (strided): walks the samples in index order, updates m / seen of its
// own bin and leaves the bin's mass in LDS; one thread then decides `ready` and, when ready, scans the masses into the cut
// points (float64, index order); one thread per bin then takes iw from the cut points.  Every address is written by
// exactly one thread: no atomics, the same bits on every run.
__global__ __launch_bounds__(256) void level_stats_kernel(const float* __restrict__ sample_loss,
                                                          const float* __restrict__ sample_w,
                                                          const long long* __restrict__ t, int B, int T, int K,
                                                          float beta, int warmup, double eps, float* __restrict__ m,
                                                          int* __restrict__ seen, unsigned long long* __restrict__ c,
                                                          float* __restrict__ iw, int* __restrict__ ready) {
    __shared__ double q[VF_LEVEL_MAX_BINS];
    __shared__ unsigned long long cut[VF_LEVEL_MAX_BINS + 1];
    __shared__ int min_seen[256];
    __shared__ int is_ready;
    int least = 0x7fffffff;
    for (int k = threadIdx.x; k < K; k += 256) {
        float sum = 0.f;
        int cnt = 0;
        for (int s = 0; s < B; ++s) {
            if (vf_level_bin(t[s], T, K) != k) continue;
            const float ws = (sample_w ? sample_w[s] : 1.0f) * sample_loss[s];
            const float r = ws * ws;
            if (!(fabsf(r) < INFINITY)) continue;        // NaN or Inf: skipped
            sum += r;
            ++cnt;
        }
        float mk = m[k];
        int sk = seen[k];
        if (cnt > 0) {
            const float mean = sum / (float)cnt;
            mk = sk == 0 ? mean : mk + (1.0f - beta) * (mean - mk);
            sk += cnt;
            m[k] = mk;
            seen[k] = sk;
        }
        q[k] = vf_level_mass(mk, vf_level_lo(k + 1, T, K) - vf_level_lo(k, T, K));
        least = sk < least ? sk : least;
    }
    min_seen[threadIdx.x] = least;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 256; ++i) least = min_seen[i] < least ? min_seen[i] : least;
        const int ok = least >= warmup && vf_level_cuts(q, T, K, eps, cut);
        is_ready = ok;
        *ready = ok;
    }
    __syncthreads();
    if (!is_ready) return;
    for (int k = threadIdx.x; k <= K; k += 256) {
        c[k] = cut[k];
        if (k < K) iw[k] = vf_level_iw(vf_level_lo(k + 1, T, K) - vf_level_lo(k, T, K), T, cut[k + 1] - cut[k]);
    }
}

// ---- dynamic thresholding / guidance rescaling (the head of this file) ----
// grid (chunks, B).  eps_g [B][3][HW] (= eps_c when !CFG); the conditional weights as compose_fwd_kernel writes them;
// part[(b * chunks + chunk) * 4 + {0..3}] = this workgroup's sums of eps_c, eps_c^2, eps_g, eps_g^2.
// FUSED_TAIL (CFG only): which tail follows, as in y0_hat_as.  The composing guided tails round guide4's expression
// differently too -- fma(g, eps_c, gm eps_u) in the ancestral bodies, fma(gm, eps_u, g eps_c) in the few-step ones -- and
// the eps written here is pinned to the tail it stands in for (g = 1 and g = 0 reduce exactly in both forms).
template <bool CFG, bool FUSED_TAIL>
__global__ __launch_bounds__(256) void compose_eps_kernel(const float* __restrict__ out, const int* __restrict__ off,
                                                          const float* __restrict__ gscale, float* __restrict__ eps_out,
                                                          float* __restrict__ weights, double* __restrict__ part,
                                                          int Cout, int HW, int maxV, int weighting) {
    __shared__ double red[4][4];
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    float g = 1.0f, gm = 0.0f;
    const float* eu = nullptr;
    if constexpr (CFG) {
        g = gscale[b];
        gm = 1.0f - g;
        eu = out + (size_t)(off[gridDim.y] + b) * Cout * HW;
    }
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        float4 mx, inv;
        const float4 ec = compose4(out, Cout, HW, v0, v1, c, p, weighting, &mx, &inv);
        float4 eg = ec;
        if constexpr (CFG) {
            const float4 u = *reinterpret_cast<const float4*>(eu + (size_t)c * HW + p);
            if constexpr (FUSED_TAIL)
                eg = make_float4(__builtin_fmaf(g, ec.x, mul_rn(gm, u.x)), __builtin_fmaf(g, ec.y, mul_rn(gm, u.y)),
                                 __builtin_fmaf(g, ec.z, mul_rn(gm, u.z)), __builtin_fmaf(g, ec.w, mul_rn(gm, u.w)));
            else
                eg = make_float4(__builtin_fmaf(gm, u.x, mul_rn(g, ec.x)), __builtin_fmaf(gm, u.y, mul_rn(g, ec.y)),
                                 __builtin_fmaf(gm, u.z, mul_rn(g, ec.z)), __builtin_fmaf(gm, u.w, mul_rn(g, ec.w)));
        }
        *reinterpret_cast<float4*>(eps_out + (size_t)b * 3 * HW + 4 * (size_t)i) = eg;
        const double c4[4] = {ec.x, ec.y, ec.z, ec.w}, g4[4] = {eg.x, eg.y, eg.z, eg.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sum[0] += c4[j];
            sum[1] += c4[j] * c4[j];
            sum[2] += g4[j];
            sum[3] += g4[j] * g4[j];
        }
        if (weights && weighting) {
            const size_t vs = (size_t)Cout * HW;
            for (int j = 0; j < maxV; ++j) {
                float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
                if (v0 + j < v1) {
                    const float4 l = *reinterpret_cast<const float4*>(out + (size_t)(v0 + j) * vs +
                                                                     (size_t)(3 + c) * HW + p);
                    w = make_float4(expf(l.x - mx.x) * inv.x, expf(l.y - mx.y) * inv.y, expf(l.z - mx.z) * inv.z,
                                    expf(l.w - mx.w) * inv.w);
                }
                *reinterpret_cast<float4*>(weights + (((size_t)b * maxV + j) * 3) * HW + 4 * (size_t)i) = w;
            }
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 4; ++q) {                            // a fixed tree per wave, then the four waves in index order
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum[q] += __shfl_xor(sum[q], o, VF_WAVE);
        if (lane == 0) red[wid][q] = sum[q];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        part[((size_t)b * gridDim.x + blockIdx.x) * 4 + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
}

// Exact selection of the order statistics k (and k + 1 when want_next) of n values given as bit patterns with the sign
// cleared: bits_at(i), i in [0, n).  One workgroup of any multiple of 64 threads; every thread gets the result.
// Four passes of 8 bits, most significant first: a 256-bin LDS histogram of the values that match the prefix found so
// far, then the bin that holds the rank.  `below` counts the values smaller than x[k], `eq` those equal to it, so
// x[k+1] == x[k] iff below + eq > k + 1 (duplicates straddling the two ranks); else x[k+1] is the smallest value above
// x[k], an integer minimum.  Counts are 32-bit integers (a bin may hold all n values); integer adds and minima
// commute, so the result does not depend on the order the LDS atomics land in.
// A wave whose active lanes all hit ONE bin -- the usual case in the exponent pass -- adds its count once.
template <class Bits>
__device__ __forceinline__ void abs_select(Bits bits_at, int n, int k, bool want_next, unsigned* hist /*[256]*/,
                                           unsigned* sh /*[4]*/, unsigned& xk, unsigned& xk1) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    unsigned prefix = 0, mask = 0, below = 0, eq = 0;
    unsigned rank = (unsigned)k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int j = tid; j < 256; j += nt) hist[j] = 0;
        __syncthreads();
        for (int base = 0; base < n; base += nt) {           // base is uniform: every lane reaches the ballots
            const int i = base + tid;
            bool act = i < n;
            const unsigned u = act ? bits_at(i) : 0u;
            act = act && (u & mask) == prefix;
            const unsigned bin = (u >> shift) & 255u;
            const unsigned long long m = __ballot(act);
            if (m != 0ull) {
                const int lead = __ffsll((long long)m) - 1;
                const unsigned lb = (unsigned)__shfl((int)bin, lead, VF_WAVE);
                const unsigned long long same = __ballot(act && bin == lb);
                if (same == m) {
                    if (lane == lead) atomicAdd(&hist[lb], (unsigned)__popcll(m));
                } else if (act) {
                    atomicAdd(&hist[bin], 1u);
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            unsigned acc = 0;
            int j = 0;
            for (; j < 255; ++j) {
                const unsigned c = hist[j];
                if (acc + c > rank) break;
                acc += c;
            }
            sh[0] = (unsigned)j;
            sh[1] = acc;
            sh[2] = hist[j];
        }
        __syncthreads();
        prefix |= sh[0] << shift;
        mask |= 255u << shift;
        rank -= sh[1];
        below += sh[1];
        eq = sh[2];
    }
    xk = xk1 = prefix;
    if (!want_next || below + eq > (unsigned)k + 1u) return;  // (uniform: every thread holds the same counts)
    if (tid == 0) sh[3] = 0xffffffffu;
    __syncthreads();
    unsigned mn = 0xffffffffu;
    for (int i = tid; i < n; i += nt) {
        const unsigned u = bits_at(i);
        if (u > prefix && u < mn) mn = u;
    }
    if (mn != 0xffffffffu) atomicMin(&sh[3], mn);
    __syncthreads();
    xk1 = sh[3];
}

// s_q = x[k] + frac (x[k+1] - x[k]); exactly x[k] where frac == 0 or the two are equal
__device__ __forceinline__ float quantile_lerp(unsigned xk, unsigned xk1, float frac) {
    const float x0 = __uint_as_float(xk);
    return frac != 0.0f ? x0 + frac * (__uint_as_float(xk1) - x0) : x0;
}

// One workgroup per sample: stat[b] = {r_b, s_b} (the head of this file).  phi <= 0: rescale off, r_b = 1 and `part` is
// not read; k < 0: threshold off, s_b = 1 and nothing is selected.  idx = t or kidx, (ta, tb) the step's table pair;
// fused: how the tail that follows rounds y0_hat (y0_hat_as: 1 the ancestral tail, 0 the few-step one).
__global__ __launch_bounds__(1024) void sample_stat_kernel(const float* __restrict__ eps, const double* __restrict__ part,
                                                           int ch, const float* __restrict__ y,
                                                           const long long* __restrict__ idx,
                                                           const float* __restrict__ ta, const float* __restrict__ tb,
                                                           float2* __restrict__ stat, int n, float phi, int k,
                                                           float frac, float cmax, int fused) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sh[4];
    __shared__ float r_sh;
    const int b = blockIdx.x;
    const bool rescale = phi > 0.0f;
    if (threadIdx.x == 0) {
        float r = 1.0f;
        if (rescale) {
            double sm[4] = {0.0, 0.0, 0.0, 0.0};
            for (int c = 0; c < ch; ++c)
                for (int q = 0; q < 4; ++q) sm[q] += part[((size_t)b * ch + c) * 4 + q];
            const double var_c = fmax(sm[1] - sm[0] * sm[0] / (double)n, 0.0);
            const double var_g = fmax(sm[3] - sm[2] * sm[2] / (double)n, 0.0);
            if (var_g > 0.0) r = (float)((double)phi * sqrt(var_c / var_g) + (1.0 - (double)phi));
        }
        r_sh = r;
    }
    __syncthreads();
    const float r = r_sh;
    float s = 1.0f;
    if (k >= 0) {
        const long long tk = idx[b];
        const float a = ta[tk], bb = tb[tk];
        const float* e = eps + (size_t)b * n;
        const float* yy = y + (size_t)b * n;
        unsigned xk, xk1;
        abs_select(
            [=](int i) {
                float ev = e[i];
                if (rescale) ev = r * ev;
                const float v = fused ? y0_hat_as<true>(a, yy[i], bb, ev) : y0_hat_as<false>(a, yy[i], bb, ev);
                return __float_as_uint(v) & 0x7fffffffu;
            },
            n, k, frac != 0.0f, hist, sh, xk, xk1);
        s = fminf(fmaxf(1.0f, quantile_lerp(xk, xk1, frac)), cmax);
    }
    if (threadIdx.x == 0) stat[b] = make_float2(r, s);
}

// out[b] = the (k, frac) quantile of |x[b][0..n)|: the same selection on a plain buffer; one workgroup per row
__global__ __launch_bounds__(1024) void abs_quantile_kernel(const float* __restrict__ x, float* __restrict__ out, int n,
                                                            int k, float frac) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sh[4];
    const float* row = x + (size_t)blockIdx.x * n;
    unsigned xk, xk1;
    abs_select([=](int i) { return __float_as_uint(row[i]) & 0x7fffffffu; }, n, k, frac != 0.0f, hist, sh, xk, xk1);
    if (threadIdx.x == 0) out[blockIdx.x] = quantile_lerp(xk, xk1, frac);
}

inline int chunks_for(int n4) {
    int c = (n4 + 255) / 256;
    return c < 1 ? 1 : (c > 64 ? 64 : c);
}

// ---- the reverse-step tails: one launcher per flavour behind twelve entry points ----
// Each entry point names its instantiation and hands its own arguments on; what its variant does not have is null / 0.
//   plain: unet_out [off[B]][Cout][HW];   _cfg: + g [B], unet_out is [off[B] + B][Cout][HW] (the null rows last);
//   _eps:  eps [B][3][HW] and stat [B][2] from vf_compose_eps / vf_sample_stat instead of unet_out;
//   _rng:  seed and ids [B] instead of z.
// What an entry refuses is what it always refused, which is not the same for every variant: a missing g only where there
// is one; HW <= 0, a missing eps and a missing stat under rescale / thr only in the _eps entries (the others launch a
// kernel with nothing to do for HW == 0); Cout only where there is a unet_out; a missing y_next only in the few-step
// entries (the ancestral kernel skips a null y_next); no other pointer is looked at.
template <bool CFG, bool EPS>
inline bool tail_args_ok(const float* eps, const float* stat, const float* g, int Cout, int HW, int weighting,
                         int rescale, int thr) {
    if (HW & 3) return false;
    if (EPS) return HW > 0 && eps && (stat || !(rescale || thr));
    return Cout >= 3 && (!weighting || Cout >= 6) && (!CFG || g);
}

template <bool CFG, bool EPS, bool RNG>
int p_sample_tail(const float* unet_out, const int* off, const float* eps, const float* stat, const float* y_t,
                  const float* z, unsigned long long seed, const long long* ids, const long long* t,
                  const float* sqrt_recip_gammas, const float* sqrt_recipm1_gammas,
                  const float* posterior_log_variance, const float* posterior_mean_coef1,
                  const float* posterior_mean_coef2, float* y_next, float* mean_out, float* weights, int B,
                  int Cout, int HW, int maxV, int weighting, int clip, const float* g, int rescale, int thr,
                  void* stream) {
    if (B <= 0) return 0;
    if (!tail_args_ok<CFG, EPS>(eps, stat, g, Cout, HW, weighting, rescale, thr)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((p_sample_tail_kernel<CFG, EPS, RNG>), dim3(chunks_for(3 * HW / 4), B), dim3(256), 0,
                       (hipStream_t)stream, unet_out, off, eps, (const float2*)stat, y_t, z, seed, ids, t,
                       sqrt_recip_gammas, sqrt_recipm1_gammas, posterior_log_variance, posterior_mean_coef1,
                       posterior_mean_coef2, y_next, mean_out, weights, Cout, HW, maxV, weighting, clip, g, rescale, thr);
    VF_RETURN_LAST_ERROR();
}

// the few-step tail (tables: schedule.sampler_tables)
template <bool CFG, bool EPS, bool RNG>
int sampler_step(const float* unet_out, const int* off, const float* eps, const float* stat, const float* y_t,
                 const float* z, unsigned long long seed, const long long* ids, const long long* kidx,
                 const long long* tau, const float* a, const float* b, const float* cy, const float* c0,
                 const float* c1, const float* sigma, float* y0_prev, float* y_next, float* weights, int B,
                 int Cout, int HW, int maxV, int weighting, const float* g, int rescale, int thr, void* stream) {
    if (B <= 0) return 0;
    if (!tail_args_ok<CFG, EPS>(eps, stat, g, Cout, HW, weighting, rescale, thr) || !y_next)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((sampler_step_kernel<CFG, EPS, RNG>), dim3(chunks_for(3 * HW / 4), B), dim3(256), 0,
                       (hipStream_t)stream, unet_out, off, eps, (const float2*)stat, y_t, z, seed, ids, kidx, tau, a, b,
                       cy, c0, c1, sigma, y0_prev, y_next, weights, Cout, HW, maxV, weighting, g, rescale, thr);
    VF_RETURN_LAST_ERROR();
}

// ---- progressive distillation (the head of this file) ----
// The student step of sample b, its two teacher steps and its level, and z_t.  grid (chunks, B); i_in (int64 [B] | null):
// an injected i, clamped to 0..K-1; else i = mulhi32(word 0 of the training-scalars call, K).  z_t is stack_views_kernel's
// q_sample expression, so the student's stacked target half -- a copy of this buffer -- carries these bits.
__global__ __launch_bounds__(256) void distill_begin_kernel(unsigned long long seed, const long long* __restrict__ ids,
                                                            const long long* __restrict__ i_in,
                                                            const long long* __restrict__ tau_s,
                                                            const float* __restrict__ gammas, int K,
                                                            const float4* __restrict__ y_0,
                                                            const float4* __restrict__ noise, long long* __restrict__ i_out,
                                                            long long* __restrict__ k1, long long* __restrict__ k0,
                                                            float* __restrict__ level_s, float4* __restrict__ z_t, int n4) {
    const int b = blockIdx.y;
    long long i;
    if (i_in != nullptr) {
        i = i_in[b];
        i = i < 0 ? 0 : (i > K - 1 ? K - 1 : i);
    } else {
        uint32_t w[4];
        vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
        i = vf_rng_distill_step(w[0], K);
    }
    const float lv = gammas[tau_s[i]];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        i_out[b] = i;
        k1[b] = 2 * i + 1;
        k0[b] = 2 * i;
        level_s[b] = lv;
    }
    const float sa = sqrtf(lv), sb = sqrtf(1.0f - lv);
    const float4* t = y_0 + (size_t)b * n4;
    const float4* z = noise + (size_t)b * n4;
    float4* o = z_t + (size_t)b * n4;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n4; j += gridDim.x * 256) {
        float4 y = t[j];
        const float4 e = z[j];
        y.x = sa * y.x + sb * e.x;
        y.y = sa * y.y + sb * e.y;
        y.z = sa * y.z + sb * e.z;
        y.w = sa * y.w + sb * e.w;
        o[j] = y;
    }
}

// The second teacher step's tail (steps 3 - 5 of the definition): out2 composed (+ guided) with the tails' own prologue,
// x2 as sampler_step_kernel forms y0 (both products rounded, then subtracted: y0_hat_as<false>), then x~ and eps~ in
// pinned arithmetic.  y = z' (the first step's y_next), x1 = the history buffer that step wrote.  One read of each
// input, one write of each output; grid (chunks, B); no atomics.
template <bool CFG>
__global__ __launch_bounds__(256) void distill_target_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ y, const float* __restrict__ x1,
    const float* __restrict__ z_t, const float* __restrict__ level_s, const long long* __restrict__ idx,
    const long long* __restrict__ kidx, const float* __restrict__ ta, const float* __restrict__ tb,
    const float* __restrict__ tw1, const float* __restrict__ tw2, float* __restrict__ x_tilde,
    float* __restrict__ eps_tilde, int Cout, int HW, int weighting, const float* __restrict__ gscale) {
    const int b = blockIdx.y;
    const TailSample s = tail_sample<CFG, false>(out, off, gscale, EpsBuffer{}, Cout, HW);
    const int n4 = 3 * HW / 4;
    const long long i = idx[b], k = kidx[b];
    const float a_k = ta[k], b_k = tb[k], w1 = tw1[i], w2 = tw2[i];
    const float lv = level_s[b];
    const float sa = sqrtf(lv), sb = sqrtf(1.0f - lv);
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n4; j += gridDim.x * 256) {
        const int c = (4 * j) / HW, p = 4 * j - c * HW;
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)j;
        const float4 eps = tail_eps<CFG, false>(s, out, EpsBuffer{}, Cout, HW, weighting, c, p, o, nullptr, nullptr);
        const float4 yy = *reinterpret_cast<const float4*>(y + o);
        const float4 h = *reinterpret_cast<const float4*>(x1 + o);
        const float4 zt = *reinterpret_cast<const float4*>(z_t + o);
        const float ys[4] = {yy.x, yy.y, yy.z, yy.w}, es[4] = {eps.x, eps.y, eps.z, eps.w};
        const float hs[4] = {h.x, h.y, h.z, h.w}, zs[4] = {zt.x, zt.y, zt.z, zt.w};
        float xt[4], et[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float x2 = fminf(fmaxf(y0_hat_as<false>(a_k, ys[q], b_k, es[q]), -1.0f), 1.0f);
            xt[q] = fminf(fmaxf(__builtin_fmaf(w1, hs[q], mul_rn(w2, x2)), -1.0f), 1.0f);
            et[q] = add_rn(zs[q], -mul_rn(sa, xt[q])) / sb;
        }
        *reinterpret_cast<float4*>(x_tilde + o) = make_float4(xt[0], xt[1], xt[2], xt[3]);
        *reinterpret_cast<float4*>(eps_tilde + o) = make_float4(et[0], et[1], et[2], et[3]);
    }
}

// ---- self-conditioning (the head of this file) ----
// keep[b] = the self-conditioning coin of sample ids[b] (rng.h: word 3 of the training-scalar call against thr)
__global__ void draw_self_cond_kernel(unsigned long long seed, const long long* __restrict__ ids, unsigned thr,
                                      unsigned char* __restrict__ keep, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t w[4];
    vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
    keep[b] = (unsigned char)vf_rng_self_cond(w[3], thr);
}

// (a, b) of x^ = a y_t - b out at the continuous level g, in fp32 (the head of this file); x0: (0, -1), not multiplied.
__host__ __device__ inline void vf_self_cond_coeffs(int pred, float g, float* a, float* b) {
    if (pred == VF_PRED_V) {
        *a = sqrtf(g);
        *b = sqrtf(1.0f - g);
    } else if (pred == VF_PRED_X0) {
        *a = 0.0f;
        *b = -1.0f;
    } else {
        *a = sqrtf(1.0f / g);
        *b = sqrtf((1.0f - g) / g);
    }
}

// x^[b] = keep[b] clamp(a y_t - b out_b, -1, 1): out_b composed with compose4 from the first pass's output, y_t read at
// y + row * y_stride + y_off (floats; row = off[b] for the stacked input, b for a plain buffer).  grid (chunks, B); one
// read of each input, one write, no atomics.  keep (uint8 [B] | null = all kept); a sample with keep = 0 gets exact zeros.
template <int PRED>
__global__ __launch_bounds__(256) void self_cond_estimate_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ level,
    const float* __restrict__ y, long long y_stride, long long y_off, int y_by_view,
    const unsigned char* __restrict__ keep, float* __restrict__ x_hat, int Cout, int HW, int weighting) {
    const int b = blockIdx.y;
    const int n4 = 3 * HW / 4;
    float* xo = x_hat + (size_t)b * 3 * HW;
    if (keep != nullptr && keep[b] == 0) {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256)
            *reinterpret_cast<float4*>(xo + 4 * (size_t)i) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int v0 = off[b], v1 = off[b + 1];
    float a_g = 0.f, b_g = -1.f;
    const float* yt = nullptr;
    if (PRED != VF_PRED_X0) {
        vf_self_cond_coeffs(PRED, level[b], &a_g, &b_g);
        yt = y + (size_t)(y_by_view ? v0 : b) * (size_t)y_stride + (size_t)y_off;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        const float4 e = compose4(out, Cout, HW, v0, v1, c, p, weighting, nullptr, nullptr);
        float r[4] = {e.x, e.y, e.z, e.w};
        if (PRED != VF_PRED_X0) {
            const float4 yy = *reinterpret_cast<const float4*>(yt + 4 * (size_t)i);
            const float ys[4] = {yy.x, yy.y, yy.z, yy.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = y0_hat_as<false>(a_g, ys[q], b_g, r[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = fminf(fmaxf(r[q], -1.0f), 1.0f);
        *reinterpret_cast<float4*>(xo + 4 * (size_t)i) = make_float4(r[0], r[1], r[2], r[3]);
    }
}

// ---- learned variance (the head of this file): the few-step tail with a per-pixel noise scale; the hybrid loss is the
// loss family's LV switch ----
// sampler_step_kernel<CFG, false, RNG> on the "ddim", eta = 1 tables with a per-pixel noise scale: y0 and cy y + c0 y0
// rounded as that kernel rounds them (y0_hat_as<false>, the guided combination and multistep_base as its instruction
// stream has them), then, where sigma[k] != 0, r = fma(expf(0.5 lp), z, r) with lp from hi[k], lo[k] and o_b -- the
// composition of the CONDITIONAL rows' channels 6..8 (the null row's are not read).  No history term: the tables' c1 is 0.
// lp_out (nullable): lp of every element, whatever sigma[k] is (p_mean_variance).
template <bool CFG, bool RNG>
__global__ __launch_bounds__(256) void sampler_step_lv_kernel(
    const float* __restrict__ out, const int* __restrict__ off, const float* __restrict__ y_t,
    const float* __restrict__ z, unsigned long long seed, const long long* __restrict__ ids,
    const long long* __restrict__ kidx, const long long* __restrict__ tau, const float* __restrict__ ta,
    const float* __restrict__ tb, const float* __restrict__ tcy, const float* __restrict__ tc0,
    const float* __restrict__ tsigma, const float* __restrict__ thi, const float* __restrict__ tlo, float* y0_prev,
    float* __restrict__ y_next, float* __restrict__ weights, float* __restrict__ lp_out, int Cout, int HW, int maxV,
    int weighting, const float* __restrict__ gscale) {
    const int b = blockIdx.y;
    const EpsBuffer src{};
    const TailSample s = tail_sample<CFG, false>(out, off, gscale, src, Cout, HW);
    const int n4 = 3 * HW / 4;
    const long long k = kidx[b];
    const auto noise = tail_noise<RNG, false>(z, seed, ids, RNG ? (uint32_t)tau[k] : 0u);
    const float a_k = ta[k], b_k = tb[k], cy = tcy[k], c0 = tc0[k], hi = thi[k], lo = tlo[k];
    const bool noisy = tsigma[k] != 0.0f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        float4 mx = make_float4(0.f, 0.f, 0.f, 0.f), inv = mx;
        float4 eps = compose4(out, Cout, HW, s.v0, s.v1, c, p, weighting, &mx, &inv);
        const float4 ob = compose4_var(out, Cout, HW, s.v0, s.v1, c, p, weighting, mx, inv);
        if constexpr (CFG) {
            const float4 u = *reinterpret_cast<const float4*>(s.eu + (size_t)c * HW + p);
            eps = make_float4(__builtin_fmaf(s.gm, u.x, mul_rn(s.g, eps.x)), __builtin_fmaf(s.gm, u.y, mul_rn(s.g, eps.y)),
                              __builtin_fmaf(s.gm, u.z, mul_rn(s.g, eps.z)), __builtin_fmaf(s.gm, u.w, mul_rn(s.g, eps.w)));
        }
        const float4 y = *reinterpret_cast<const float4*>(y_t + o);
        const float ys[4] = {y.x, y.y, y.z, y.w};
        const float es[4] = {eps.x, eps.y, eps.z, eps.w};
        const float os[4] = {ob.x, ob.y, ob.z, ob.w};
        float y0[4], r[4], lp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            y0[j] = fminf(fmaxf(y0_hat_as<false>(a_k, ys[j], b_k, es[j]), -1.0f), 1.0f);
            r[j] = multistep_base<true>(cy, ys[j], c0, y0[j], j);
            lp[j] = vf_vlb_logvar(os[j], hi, lo);
        }
        if (noisy) {
            const float4 zz = noise(i, o);
            const float zs[4] = {zz.x, zz.y, zz.z, zz.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = __builtin_fmaf(expf(mul_rn(0.5f, lp[j])), zs[j], r[j]);
        }
        if (y0_prev) *reinterpret_cast<float4*>(y0_prev + o) = make_float4(y0[0], y0[1], y0[2], y0[3]);
        *reinterpret_cast<float4*>(y_next + o) = make_float4(r[0], r[1], r[2], r[3]);
        if (lp_out) *reinterpret_cast<float4*>(lp_out + o) = make_float4(lp[0], lp[1], lp[2], lp[3]);
        if (weights && weighting) write_weights(out, weights, Cout, HW, maxV, s.v0, s.v1, c, p, i, mx, inv);
    }
}

// the one launcher of the learned-variance tail behind its four entry points; it holds the argument check
template <bool CFG, bool RNG>
int sampler_step_lv(const float* unet_out, const int* off, const float* y_t, const float* z, unsigned long long seed,
                    const long long* ids, const long long* kidx, const long long* tau, const float* a, const float* b,
                    const float* cy, const float* c0, const float* sigma, const float* hi, const float* lo,
                    float* y0_prev, float* y_next, float* weights, float* lp_out, int B, int Cout, int HW, int maxV,
                    int weighting, const float* g, void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || HW <= 0 || Cout < 9 || (CFG && !g) || (RNG && (!ids || !tau))) return (int)hipErrorInvalidValue;
    if (!unet_out || !off || !y_t || !kidx || !a || !b || !cy || !c0 || !sigma || !hi || !lo || !y_next)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((sampler_step_lv_kernel<CFG, RNG>), dim3(chunks_for(3 * HW / 4), B), dim3(256), 0,
                       (hipStream_t)stream, unet_out, off, y_t, z, seed, ids, kidx, tau, a, b, cy, c0, sigma, hi, lo,
                       y0_prev, y_next, weights, lp_out, Cout, HW, maxV, weighting, g);
    VF_RETURN_LAST_ERROR();
}

// ---- the loss family: LV and the run-time (penalty, pred) -> the kernel pair (the launchers stand with the entry
// points) ----
template <bool LV>
struct LossKernels {
    decltype(&compose_loss_fwd_kernel<VF_LOSS_MSE, VF_PRED_EPS, LV>) fwd;
    decltype(&compose_loss_bwd_kernel<VF_LOSS_MSE, VF_PRED_EPS, LV>) bwd;
};

template <int PRED, bool LV>
LossKernels<LV> loss_kernels_of(int penalty) {
    if (penalty == VF_LOSS_L1)
        return {compose_loss_fwd_kernel<VF_LOSS_L1, PRED, LV>, compose_loss_bwd_kernel<VF_LOSS_L1, PRED, LV>};
    if (penalty == VF_LOSS_HUBER)
        return {compose_loss_fwd_kernel<VF_LOSS_HUBER, PRED, LV>, compose_loss_bwd_kernel<VF_LOSS_HUBER, PRED, LV>};
    return {compose_loss_fwd_kernel<VF_LOSS_MSE, PRED, LV>, compose_loss_bwd_kernel<VF_LOSS_MSE, PRED, LV>};
}

// the run-time (penalty, pred) -> the instantiation: the one place that names the eighteen of each
template <bool LV>
LossKernels<LV> loss_kernels(int penalty, int pred) {
    if (pred == VF_PRED_V) return loss_kernels_of<VF_PRED_V, LV>(penalty);
    if (pred == VF_PRED_X0) return loss_kernels_of<VF_PRED_X0, LV>(penalty);
    return loss_kernels_of<VF_PRED_EPS, LV>(penalty);
}

// ---- the variational bound (the head of this file holds the definition, vlb.h the arithmetic) ----
// One element of one term: y0 = clamp(a y - b out) (both products rounded, then subtracted, as the few-step tails form
// it), d = y0 - x, sq = d d, and the term in bits -- the decoder likelihood of x under N(y0, exp(lp)) with DEC, else the
// KL of vlb.h at m^2 = c0^2 d^2.  The kernel and the host mirror (vf_nll_terms_host) both run this very function.
struct NllRow {
    float a, b, c0, hi, lo;
};
template <bool DEC>
__host__ __device__ inline float nll_element(const NllRow& r, float out, float lp, float y, float x, int clip,
                                             float* sq) {
#pragma clang fp contract(off)
    const float ay = r.a * y;
    const float bo = r.b * out;
    float y0 = ay - bo;
    if (clip) y0 = fminf(fmaxf(y0, -1.0f), 1.0f);
    const float d = y0 - x;
    *sq = d * d;
    if (DEC) return vf_nll_decoder(x, y0, lp);
    return vf_vlb_kl(lp, r.lo, vf_vlb_m2(r.c0, 1.0f, d));
}

// The step index of a sample, clamped into the chain before any table is read.
__device__ __forceinline__ long long nll_step(const long long* __restrict__ kidx, int b, int K) {
    const long long k = kidx[b];
    return k < 0 ? 0 : (k > K - 1 ? K - 1 : k);
}

// The noisy target of step k = kidx[b]: y_k = sqrt(g) y_0 + sqrt(1 - g) n, g = gammas[tau[k]], both products rounded, then
// added.  RNG: n is drawn here, kind 6, step = tau[k], block = the float4 index, keyed by the sample's id; else loaded
// from noise[B][K][3][HW] at (b, k).  grid (chunks, B).
template <bool RNG>
__global__ __launch_bounds__(256) void nll_noisy_kernel(const float* __restrict__ y_0, const float* __restrict__ noise,
                                                        unsigned long long seed, const long long* __restrict__ ids,
                                                        const long long* __restrict__ kidx,
                                                        const long long* __restrict__ tau,
                                                        const float* __restrict__ gammas, float* __restrict__ y_k,
                                                        int HW, int K, int T) {
    const int b = blockIdx.y;
    const int n4 = 3 * HW / 4;
    const long long k = nll_step(kidx, b, K);
    long long t = tau[k];
    t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
    const float g = gammas[t];
    const float sa = sqrtf(g), sb = sqrtf(1.0f - g);
    unsigned long long id = 0;
    if constexpr (RNG) id = (unsigned long long)ids[b];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        const float4 x = *reinterpret_cast<const float4*>(y_0 + o);
        float n[4];
        if constexpr (RNG) {
            vf_rng_normal4(seed, id, VF_RNG_NLL_NOISE, (uint32_t)t, (uint32_t)i, n);
        } else {
            const float4 z = *reinterpret_cast<const float4*>(noise + ((size_t)b * K + (size_t)k) * 3 * HW +
                                                              4 * (size_t)i);
            n[0] = z.x; n[1] = z.y; n[2] = z.z; n[3] = z.w;
        }
        *reinterpret_cast<float4*>(y_k + o) =
            make_float4(add_rn(mul_rn(sa, x.x), mul_rn(sb, n[0])), add_rn(mul_rn(sa, x.y), mul_rn(sb, n[1])),
                        add_rn(mul_rn(sa, x.z), mul_rn(sb, n[2])), add_rn(mul_rn(sa, x.w), mul_rn(sb, n[3])));
    }
}

// One term of the bound per (b, chunk): compose_loss_fwd_kernel's geometry and composition, the row k = kidx[b] of the
// tables, the term and (y0 - y_0)^2 in registers, two partial sums.  LV: lp between lo[k] and hi[k] by the composed
// channels 6..8; else lp = hi[k] where `large`, lo[k] otherwise.  DEC: the decoder likelihood (the launcher's k == 0).
template <bool LV, bool DEC>
__global__ __launch_bounds__(256) void nll_term_kernel(const float* __restrict__ out, const int* __restrict__ off,
                                                       const float* __restrict__ y_k, const float* __restrict__ y_0,
                                                       const long long* __restrict__ kidx, const float* __restrict__ ta,
                                                       const float* __restrict__ tb, const float* __restrict__ tc0,
                                                       const float* __restrict__ thi, const float* __restrict__ tlo,
                                                       float* __restrict__ vb_part, float* __restrict__ sq_part,
                                                       int Cout, int HW, int K, int weighting, int clip, int large) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    const long long k = nll_step(kidx, b, K);
    const NllRow row{ta[k], tb[k], tc0[k], thi[k], tlo[k]};
    const float lp_fixed = large ? row.hi : row.lo;
    float acc = 0.f, sq = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        float4 mx = make_float4(0.f, 0.f, 0.f, 0.f), inv = mx, ob = mx;
        const float4 e = compose4(out, Cout, HW, v0, v1, c, p, weighting, LV ? &mx : nullptr, LV ? &inv : nullptr);
        if constexpr (LV) ob = compose4_var(out, Cout, HW, v0, v1, c, p, weighting, mx, inv);
        const size_t o = (size_t)b * 3 * HW + 4 * (size_t)i;
        const float4 y = *reinterpret_cast<const float4*>(y_k + o);
        const float4 x = *reinterpret_cast<const float4*>(y_0 + o);
        const float es[4] = {e.x, e.y, e.z, e.w}, os[4] = {ob.x, ob.y, ob.z, ob.w};
        const float ys[4] = {y.x, y.y, y.z, y.w}, xs[4] = {x.x, x.y, x.z, x.w};
        float t[4], s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float lp = LV ? vf_vlb_logvar(os[j], row.hi, row.lo) : lp_fixed;
            t[j] = nll_element<DEC>(row, es[j], lp, ys[j], xs[j], clip, &s[j]);
        }
        acc += (t[0] + t[1]) + (t[2] + t[3]);
        sq += (s[0] + s[1]) + (s[2] + s[3]);
    }
    acc = block_sum<256>(acc, red);
    sq = block_sum<256>(sq, red);
    if (threadIdx.x == 0) {
        vb_part[blockIdx.y * gridDim.x + blockIdx.x] = acc;
        sq_part[blockIdx.y * gridDim.x + blockIdx.x] = sq;
    }
}

// The prior term per (b, chunk): 0.5 (-1 - log(1 - gT) + (1 - gT) + gT y_0^2) / ln 2 with gT = gammas[T - 1]; gT == 0
// gives 0 exactly.
__global__ __launch_bounds__(256) void nll_prior_kernel(const float* __restrict__ y_0, const float* __restrict__ gammas,
                                                        float* __restrict__ part, int HW, int T) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const int n4 = 3 * HW / 4;
    const float gT = gammas[T - 1];
    const float om = 1.0f - gT;
    const float base = add_rn(add_rn(-1.0f, -logf(om)), om);
    float acc = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const float4 x = *reinterpret_cast<const float4*>(y_0 + (size_t)b * 3 * HW + 4 * (size_t)i);
        const float xs[4] = {x.x, x.y, x.z, x.w};
        float t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            t[j] = mul_rn(mul_rn(0.5f, add_rn(base, mul_rn(gT, mul_rn(xs[j], xs[j])))), VF_VLB_INV_LN2);
        acc += (t[0] + t[1]) + (t[2] + t[3]);
    }
    acc = block_sum<256>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// One thread per sample: its `ch` partials in index order, / n, into column k = kidx[b] of the (B, K) tables (kidx null:
// column 0; sq_part / x0_mse null: the one table).  Every address is written by exactly one thread: the same bits on
// every run, whatever the batch.
__global__ __launch_bounds__(64) void nll_finish_kernel(const float* __restrict__ vb_part,
                                                        const float* __restrict__ sq_part,
                                                        const long long* __restrict__ kidx, float* __restrict__ vb,
                                                        float* __restrict__ x0_mse, int B, int ch, int K, float inv_n) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= B) return;
    const long long k = kidx ? nll_step(kidx, s, K) : 0;
    float acc = 0.f;
    for (int c = 0; c < ch; ++c) acc += vb_part[s * ch + c];
    vb[(size_t)s * K + k] = acc * inv_n;
    if (sq_part != nullptr) {
        float sq = 0.f;
        for (int c = 0; c < ch; ++c) sq += sq_part[s * ch + c];
        x0_mse[(size_t)s * K + k] = sq * inv_n;
    }
}

// ---- the analytic variance (the head of this file holds the definition) ----
// One element of the noise estimate: e = ea y + eb out, both products rounded, then added; returns e^2.  The kernel and
// the host mirror (vf_eps_moment_host) both run this very function.
__host__ __device__ inline float eps_moment_element(float ea, float eb, float out, float y, float* eps) {
#pragma clang fp contract(off)
    const float ay = ea * y;
    const float bo = eb * out;
    const float e = ay + bo;
    *eps = e;
    return e * e;
}

// The sum of e^2 per (b, chunk): nll_term_kernel's geometry and composition (channels 0..2 under the softmax of 3..5, or
// the mean; channels 6.. are never read), the row k = kidx[b] of the two tables, one partial sum.
__global__ __launch_bounds__(256) void eps_moment_kernel(const float* __restrict__ out, const int* __restrict__ off,
                                                         const float* __restrict__ y_k,
                                                         const long long* __restrict__ kidx,
                                                         const float* __restrict__ tea, const float* __restrict__ teb,
                                                         float* __restrict__ part, int Cout, int HW, int K,
                                                         int weighting) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const int v0 = off[b], v1 = off[b + 1];
    const int n4 = 3 * HW / 4;
    const long long k = nll_step(kidx, b, K);
    const float ea = tea[k], eb = teb[k];
    float acc = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int c = (4 * i) / HW, p = 4 * i - c * HW;
        const float4 e = compose4(out, Cout, HW, v0, v1, c, p, weighting, nullptr, nullptr);
        const float4 y = *reinterpret_cast<const float4*>(y_k + (size_t)b * 3 * HW + 4 * (size_t)i);
        const float es[4] = {e.x, e.y, e.z, e.w}, ys[4] = {y.x, y.y, y.z, y.w};
        float t[4], eps;
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = eps_moment_element(ea, eb, es[j], ys[j], &eps);
        acc += (t[0] + t[1]) + (t[2] + t[3]);
    }
    acc = block_sum<256>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

}  // namespace

extern "C" {

int vf_psnr(const float* generated, const float* target, float* out, int B, int n, void* stream) {
    if (B <= 0) return 0;
    if (n & 3) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(psnr_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, generated, target, out, n);
    VF_RETURN_LAST_ERROR();
}

int vf_gather_level(const float* gammas, const long long* t, const float* u, float* level, int B, void* stream) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(gather_level_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, gammas, t, u,
                       level, B);
    VF_RETURN_LAST_ERROR();
}

// y_cond [B][Nmax][3][HW], y_t [B][3][HW], noise [B][3][HW] or null, level/angle [B],
// off [B+1] -> x [S][6][HW], level_s/angle_s [S].
int vf_stack_views(const float* y_cond, const float* y_t, const float* noise, const float* level,
                   const float* angle, const int* off, float* x, float* level_s, float* angle_s, int B, int Nmax,
                   int Cc, int HW, int S, int copy_cond, void* stream) {
    if (S <= 0) return 0;
    if ((HW & 3) || Cc < 1) return (int)hipErrorInvalidValue;
    const int n4 = 3 * HW / 4, nc4 = Cc * HW / 4;
    hipLaunchKernelGGL(stack_views_kernel, dim3(chunks_for(nc4 > n4 ? nc4 : n4), S), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)y_cond, (const float4*)y_t, (const float4*)noise, level, angle, off,
                       (float4*)x, level_s, angle_s, B, Nmax, nc4, n4, copy_cond);
    VF_RETURN_LAST_ERROR();
}

// loss_part must hold B*64 floats when target != null.
int vf_compose_fwd(const float* unet_out, const int* off, const float* target, float* noise_hat, float* weights,
                   float* loss_part, float* loss, int B, int Cout, int HW, int maxV, int weighting, void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || Cout < 3 || (weighting && Cout < 6)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int ch = chunks_for(3 * HW / 4);
    hipLaunchKernelGGL(compose_fwd_kernel, dim3(ch, B), dim3(256), 0, st, unet_out, off, target, noise_hat, weights,
                       target ? loss_part : nullptr, Cout, HW, maxV, weighting);
    if (target)
        hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(64), 0, st, loss_part, loss, B * ch,
                           1.0f / ((float)B * 3.0f * (float)HW));
    VF_RETURN_LAST_ERROR();
}

int vf_compose_mse_bwd(const float* unet_out, const int* off, const float* target, const float* noise_hat,
                       const float* gloss, float* dout, int B, int Cout, int HW, int weighting, void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || Cout < 3 || (weighting && Cout < 6)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(compose_mse_bwd_kernel, dim3(chunks_for(3 * HW / 4), B), dim3(256), 0, (hipStream_t)stream,
                       unet_out, off, target, noise_hat, gloss, dout, Cout, HW, weighting,
                       1.0f / ((float)B * 3.0f * (float)HW));
    VF_RETURN_LAST_ERROR();
}

// ---- the loss family (loss_weight.h): vf_compose_fwd with a target / vf_compose_mse_bwd with a penalty, a prediction, a
// per-sample weight of `level` (times a per-sample scale), the per-sample loss and an optional histogram.  Two launches
// forward, one backward, as those.  Five entry points in front of one forward and one backward launcher (and the two of
// the hybrid loss, vf_compose_loss_lv_fwd / _bwd, which stand with the learned-variance entries further down):
//   vf_compose_loss_fwd          eps, the target ready-made;
//   vf_compose_loss_fwd_scaled   + scale (DEVICE float [B], the importance weight of level_sampler.h): sample_w then holds
//                                2 B floats, w_b scale_b (what the loss and the backward use) and then w_b alone;
//                                scale == NULL is vf_compose_loss_fwd itself;
//   vf_compose_loss_bwd          eps;
//   vf_compose_loss_pred_fwd / _pred_bwd   pred 1 (v) | 2 (x0), fed noise, y_0 and level instead of a target; scale
//                                (nullable) as above; noise may be NULL for x0; pred 0 (eps) is refused: its path is the
//                                entries above.
// What an entry refuses is what it always refused, which is not the same for every entry.  All: B <= 0 returns 0 without a
// launch; HW & 3, Cout < 3, weighting with Cout < 6, an unknown penalty, huber with delta <= 0; a null sample_w.  The three
// forward entries: an unknown weight_kind, bin_sum without bin_cnt or the reverse, bins with K < 1, a null level, noise_hat,
// loss_part, sample_loss or loss.  The eps forward entries: a null target.  The pred entries: pred other than 1 | 2, a null
// y_0, a null noise for v; vf_compose_loss_pred_bwd alone also a null level, noise_hat, gloss or dout --
// vf_compose_loss_bwd looks at no pointer but sample_w. ----
static inline bool loss_args_ok(int Cout, int HW, int weighting, int penalty, float delta) {
    if ((HW & 3) || Cout < 3 || (weighting && Cout < 6)) return false;
    if (penalty < VF_LOSS_MSE || penalty > VF_LOSS_HUBER) return false;
    return penalty != VF_LOSS_HUBER || delta > 0.0f;
}

static inline bool pred_args_ok(int pred, const float* noise, const float* y_0) {
    return (pred == VF_PRED_V || pred == VF_PRED_X0) && y_0 && (pred == VF_PRED_X0 || noise);
}

// noise: the ready-made target for pred 0 (y_0 is then not read).  LV: the hybrid loss -- its operands for the forward
// and the finish kernel (checked by its entry), and scale is null; the five older entries call loss_fwd<false>.
extern "C++" {          // (templates, in the middle of the C entry points they serve)
template <bool LV = false>
static int loss_fwd(int pred, const float* unet_out, const int* off, const float* noise, const float* y_0,
                    const float* level, const float* scale, float* noise_hat, float* loss_part, float* sample_loss,
                    float* sample_w, float* loss, float* bin_sum, int* bin_cnt, int B, int Cout, int HW, int weighting,
                    int penalty, float delta, int weight_kind, float a, float b, int K, void* stream,
                    VlbFwd<LV> fwd_vo = {}, VlbFinish<LV> fin_vo = {}) {
    if (B <= 0) return 0;
    if (!loss_args_ok(Cout, HW, weighting, penalty, delta)) return (int)hipErrorInvalidValue;
    if (weight_kind < VF_LOSS_W_NONE || weight_kind > VF_LOSS_W_LAST) return (int)hipErrorInvalidValue;
    if ((bin_sum == nullptr) != (bin_cnt == nullptr) || (bin_sum && K < 1)) return (int)hipErrorInvalidValue;
    if (!level || !noise_hat || !loss_part || !sample_loss || !sample_w || !loss) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int ch = chunks_for(3 * HW / 4);
    hipLaunchKernelGGL(loss_kernels<LV>(penalty, pred).fwd, dim3(ch, B), dim3(256), 0, st, unet_out, off, noise, y_0,
                       level, noise_hat, loss_part, Cout, HW, weighting, delta, fwd_vo);
    hipLaunchKernelGGL(compose_loss_finish_kernel<LV>, dim3(1), dim3(64), 0, st, loss_part, level, scale, sample_loss,
                       sample_w, loss, bin_sum, bin_cnt, B, ch, K, 1.0f / (3.0f * (float)HW), weight_kind, a, b, pred,
                       fin_vo);
    VF_RETURN_LAST_ERROR();
}

template <bool LV = false>
static int loss_bwd(int pred, const float* unet_out, const int* off, const float* noise, const float* y_0,
                    const float* level, const float* noise_hat, const float* gloss, const float* sample_w, float* dout,
                    int B, int Cout, int HW, int weighting, int penalty, float delta, void* stream,
                    VlbBwd<LV> vo = {}) {
    if (B <= 0) return 0;
    if (!loss_args_ok(Cout, HW, weighting, penalty, delta) || !sample_w) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(loss_kernels<LV>(penalty, pred).bwd, dim3(chunks_for(3 * HW / 4), B), dim3(256), 0,
                       (hipStream_t)stream, unet_out, off, noise, y_0, level, noise_hat, gloss, sample_w, dout, Cout, HW,
                       weighting, 1.0f / ((float)B * 3.0f * (float)HW), delta, vo);
    VF_RETURN_LAST_ERROR();
}
}  // extern "C++"

int vf_compose_loss_fwd(const float* unet_out, const int* off, const float* target, const float* level,
                        float* noise_hat, float* loss_part, float* sample_loss, float* sample_w, float* loss,
                        float* bin_sum, int* bin_cnt, int B, int Cout, int HW, int weighting, int penalty, float delta,
                        int weight_kind, float a, float b, int K, void* stream) {
    if (B > 0 && !target) return (int)hipErrorInvalidValue;
    return loss_fwd(VF_PRED_EPS, unet_out, off, target, nullptr, level, nullptr, noise_hat, loss_part, sample_loss,
                    sample_w, loss, bin_sum, bin_cnt, B, Cout, HW, weighting, penalty, delta, weight_kind, a, b, K, stream);
}

int vf_compose_loss_fwd_scaled(const float* unet_out, const int* off, const float* target, const float* level,
                               const float* scale, float* noise_hat, float* loss_part, float* sample_loss,
                               float* sample_w, float* loss, float* bin_sum, int* bin_cnt, int B, int Cout, int HW,
                               int weighting, int penalty, float delta, int weight_kind, float a, float b, int K,
                               void* stream) {
    if (B > 0 && !target) return (int)hipErrorInvalidValue;
    return loss_fwd(VF_PRED_EPS, unet_out, off, target, nullptr, level, scale, noise_hat, loss_part, sample_loss, sample_w,
                    loss, bin_sum, bin_cnt, B, Cout, HW, weighting, penalty, delta, weight_kind, a, b, K, stream);
}

int vf_compose_loss_bwd(const float* unet_out, const int* off, const float* target, const float* noise_hat,
                        const float* gloss, const float* sample_w, float* dout, int B, int Cout, int HW, int weighting,
                        int penalty, float delta, void* stream) {
    return loss_bwd(VF_PRED_EPS, unet_out, off, target, nullptr, nullptr, noise_hat, gloss, sample_w, dout, B, Cout, HW,
                    weighting, penalty, delta, stream);
}

int vf_compose_loss_pred_fwd(const float* unet_out, const int* off, const float* noise, const float* y_0,
                             const float* level, const float* scale, float* noise_hat, float* loss_part,
                             float* sample_loss, float* sample_w, float* loss, float* bin_sum, int* bin_cnt, int B,
                             int Cout, int HW, int weighting, int penalty, float delta, int weight_kind, float a, float b,
                             int K, int pred, void* stream) {
    if (B > 0 && !pred_args_ok(pred, noise, y_0)) return (int)hipErrorInvalidValue;
    return loss_fwd(pred, unet_out, off, noise, y_0, level, scale, noise_hat, loss_part, sample_loss, sample_w, loss,
                    bin_sum, bin_cnt, B, Cout, HW, weighting, penalty, delta, weight_kind, a, b, K, stream);
}

int vf_compose_loss_pred_bwd(const float* unet_out, const int* off, const float* noise, const float* y_0,
                             const float* level, const float* noise_hat, const float* gloss, const float* sample_w,
                             float* dout, int B, int Cout, int HW, int weighting, int penalty, float delta, int pred,
                             void* stream) {
    if (B > 0 && (!pred_args_ok(pred, noise, y_0) || !level || !noise_hat || !gloss || !dout))
        return (int)hipErrorInvalidValue;
    return loss_bwd(pred, unet_out, off, noise, y_0, level, noise_hat, gloss, sample_w, dout, B, Cout, HW, weighting,
                    penalty, delta, stream);
}

// ---- loss-aware noise-level sampling (level_sampler.h) ----
// Either (seed, ids) or words (DEVICE int64 [B], values in [0, 2^32)); c [K + 1], iw [K], ready [1] in device memory.
// u / level: seeded path only, both optional.
int vf_draw_level(unsigned long long seed, const long long* ids, const long long* words, const float* gammas, int T,
                  int K, const unsigned long long* c, const float* iw, const int* ready, long long* t, float* u,
                  float* level, float* iw_out, int B, void* stream) {
    if (B <= 0) return 0;
    if (!vf_level_args_ok(T, K) || (ids == nullptr) == (words == nullptr)) return (int)hipErrorInvalidValue;
    if (!c || !iw || !ready || !t || !iw_out || (level && !gammas) || (!ids && (u || level)))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(draw_level_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, seed, ids, words, gammas,
                       T, K, c, iw, ready, t, u, level, iw_out, B);
    VF_RETURN_LAST_ERROR();
}

// One step's statistics into m / seen [K], then ready and (when ready) c [K + 1] / iw [K].  sample_w NULL: w = 1.
int vf_level_stats(const float* sample_loss, const float* sample_w, const long long* t, int B, int T, int K, float beta,
                   int warmup, double eps, float* m, int* seen, unsigned long long* c, float* iw, int* ready,
                   void* stream) {
    if (B <= 0) return 0;
    if (!vf_level_args_ok(T, K) || !(beta >= 0.0f && beta < 1.0f) || warmup < 0) return (int)hipErrorInvalidValue;
    if (!(eps * 4294967296.0 >= 2.0 * (double)(T - 1)) || !(eps <= 1.0)) return (int)hipErrorInvalidValue;
    if (!sample_loss || !t || !m || !seen || !c || !iw || !ready) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(level_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sample_loss, sample_w, t, B, T, K,
                       beta, warmup, eps, m, seen, c, iw, ready);
    VF_RETURN_LAST_ERROR();
}

// Host mirrors: the functions of level_sampler.h on the CPU.  HOST pointers, no stream.
// masses q [K] (>= 0, finite positive sum) -> c [K + 1], lo [K + 1] (lo[K] = T), iw [K]
int vf_level_table_host(const double* q, int T, int K, double eps, unsigned long long* c, int* lo, float* iw) {
    if (!vf_level_args_ok(T, K) || !(eps * 4294967296.0 >= 2.0 * (double)(T - 1)) || !(eps <= 1.0))
        return (int)hipErrorInvalidValue;
    for (int k = 0; k < K; ++k)
        if (!(q[k] >= 0.0)) return (int)hipErrorInvalidValue;
    if (!vf_level_cuts(q, T, K, eps, c)) return (int)hipErrorInvalidValue;
    for (int k = 0; k <= K; ++k) lo[k] = vf_level_lo(k, T, K);
    for (int k = 0; k < K; ++k) iw[k] = vf_level_iw(lo[k + 1] - lo[k], T, c[k + 1] - c[k]);
    return 0;
}

// words x [n] + the table -> t [n], iw_out [n] (the `ready` draw)
int vf_level_draw_host(const unsigned* x, int n, int T, int K, const unsigned long long* c, const float* iw,
                       long long* t, float* iw_out) {
    if (n < 0 || !vf_level_args_ok(T, K) || c[0] != 0 || c[K] != (1ull << 32)) return (int)hipErrorInvalidValue;
    for (int k = 0; k < K; ++k)
        if (c[k + 1] <= c[k]) return (int)hipErrorInvalidValue;
    for (int i = 0; i < n; ++i) {
        int k;
        t[i] = vf_level_draw(x[i], c, T, K, &k);
        iw_out[i] = iw[k];
    }
    return 0;
}

// Host mirror: vf_loss_weight itself on the CPU.  HOST pointers, no stream.
int vf_loss_weights_host(const float* level, int B, int kind, float a, float b, float* out) {
    if (B < 0 || kind < VF_LOSS_W_NONE || kind > VF_LOSS_W_P2) return (int)hipErrorInvalidValue;
    for (int s = 0; s < B; ++s) out[s] = vf_loss_weight(kind, a, b, level[s]);
    return 0;
}

// Host mirror: vf_loss_weight_pred itself on the CPU (pred 0 | 1 | 2).  HOST pointers, no stream.
int vf_loss_weights_pred_host(const float* level, int B, int pred, int kind, float a, float b, float* out) {
    if (B < 0 || kind < VF_LOSS_W_NONE || kind > VF_LOSS_W_P2 || pred < VF_PRED_EPS || pred > VF_PRED_X0)
        return (int)hipErrorInvalidValue;
    for (int s = 0; s < B; ++s) out[s] = vf_loss_weight_pred(pred, kind, a, b, level[s]);
    return 0;
}

// ---- seeded draws (rng.h) ----
// (kinds 0..3, and 6 -- the noisy targets of the variational bound -- whose layout these two launches share; 4 and 5 have
// launches of their own)
static inline bool rng_args_ok(int kind, int step) {
    return ((kind >= 0 && kind <= 3) || kind == VF_RNG_NLL_NOISE) && step >= 0 && step < (1 << 28);
}

int vf_draw_train(unsigned long long seed, const long long* ids, const float* gammas, int T, long long* t, float* u,
                  float* level, int B, void* stream) {
    if (B <= 0) return 0;
    if (T < 2 || T > (1 << 28)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(draw_train_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, seed, ids, gammas, T,
                       t, u, level, B);
    VF_RETURN_LAST_ERROR();
}

int vf_randn_ids(unsigned long long seed, const long long* ids, int kind, int step, float* out, int B, int n,
                 void* stream) {
    if (B <= 0 || n == 0) return 0;
    if (n < 0 || (n & 3) || !rng_args_ok(kind, step)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(randn_ids_kernel, dim3(chunks_for(n / 4), B), dim3(256), 0, (hipStream_t)stream, seed, ids, kind,
                       step, (float4*)out, n / 4);
    VF_RETURN_LAST_ERROR();
}

int vf_philox_ids(unsigned long long seed, const long long* ids, int kind, int step, unsigned* out, int B, int n,
                  void* stream) {
    if (B <= 0 || n == 0) return 0;
    if (n < 0 || (n & 3) || !rng_args_ok(kind, step)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(philox_ids_kernel, dim3(chunks_for(n / 4), B), dim3(256), 0, (hipStream_t)stream, seed, ids, kind,
                       step, (uint4*)out, n / 4);
    VF_RETURN_LAST_ERROR();
}

// ---- classifier-free guidance (the head of this file): conditioning dropout, null rows ----
// vf_stack_views with drop (DEVICE uint8 [B] | NULL) and null_rows: x [S (+ B)][Cc+3][HW], level_s / angle_s [S (+ B)].
int vf_stack_views_cfg(const float* y_cond, const float* y_t, const float* noise, const float* level,
                       const float* angle, const int* off, const unsigned char* drop, float* x, float* level_s,
                       float* angle_s, int B, int Nmax, int Cc, int HW, int S, int copy_cond, int null_rows,
                       void* stream) {
    if (S <= 0 || B <= 0) return 0;
    // a null row stands next to a sample's real rows: with null_rows every sample has at least one (S >= B); a
    // drop-only call takes any S, like vf_stack_views
    if ((HW & 3) || Cc < 1 || (null_rows && S < B)) return (int)hipErrorInvalidValue;
    const int rows = null_rows ? S + B : S;
    if (rows > 65535) return (int)hipErrorInvalidValue;
    const int n4 = 3 * HW / 4, nc4 = Cc * HW / 4;
    hipLaunchKernelGGL(stack_views_cfg_kernel<false>, dim3(chunks_for(nc4 > n4 ? nc4 : n4), rows), dim3(256), 0,
                       (hipStream_t)stream, (const float4*)y_cond, (const float4*)y_t, (const float4*)noise, level, angle,
                       off, drop, (float4*)x, level_s, angle_s, B, Nmax, nc4, n4, copy_cond, S, (const float4*)nullptr);
    VF_RETURN_LAST_ERROR();
}

int vf_draw_cond_drop(unsigned long long seed, const long long* ids, unsigned thr, unsigned char* drop, int B,
                      void* stream) {
    if (B <= 0) return 0;
    if (thr > (1u << 24)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(draw_cond_drop_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, seed, ids, thr,
                       drop, B);
    VF_RETURN_LAST_ERROR();
}

// ---- dynamic thresholding / guidance rescaling (the head of this file) ----
// eps [B][3][HW]; part: DEVICE double [B * 64 * 4]; g NULL: unguided (eps_g = eps_c, unet_out has off[B] rows);
// fused: which tail follows (1 vf_p_sample_tail_eps(_rng), 0 vf_sampler_step_eps(_rng)), as in vf_sample_stat.
int vf_compose_eps(const float* unet_out, const int* off, const float* g, float* eps, float* weights, double* part,
                   int B, int Cout, int HW, int maxV, int weighting, int fused, void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || Cout < 3 || (weighting && Cout < 6) || !eps || !part) return (int)hipErrorInvalidValue;
    const dim3 grid(chunks_for(3 * HW / 4), B), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (g && fused)
        hipLaunchKernelGGL((compose_eps_kernel<true, true>), grid, block, 0, st, unet_out, off, g, eps, weights, part,
                           Cout, HW, maxV, weighting);
    else if (g)
        hipLaunchKernelGGL((compose_eps_kernel<true, false>), grid, block, 0, st, unet_out, off, g, eps, weights, part,
                           Cout, HW, maxV, weighting);
    else
        hipLaunchKernelGGL((compose_eps_kernel<false, false>), grid, block, 0, st, unet_out, off, g, eps, weights, part,
                           Cout, HW, maxV, weighting);
    VF_RETURN_LAST_ERROR();
}

// stat [B][2] = {r_b, s_b}.  phi <= 0: no rescale; k < 0: no threshold; cmax: the cap on s_b (+inf for none).
// idx = t (ta, tb = sqrt_recip_gammas, sqrt_recipm1_gammas; fused = 1) or kidx (ta, tb = the plan's a, b; fused = 0).
int vf_sample_stat(const float* eps, const double* part, const float* y, const long long* idx, const float* ta,
                   const float* tb, float* stat, int B, int HW, float phi, int k, float frac, float cmax, int fused,
                   void* stream) {
    if (B <= 0) return 0;
    const long long n = 3ll * HW;
    if (HW <= 0 || (HW & 3) || n > 0x7fffffffll || !stat || !eps || !y) return (int)hipErrorInvalidValue;
    if (phi > 0.0f && (!part || !(phi <= 1.0f))) return (int)hipErrorInvalidValue;
    if (k >= 0 && (k >= n || !(frac >= 0.0f && frac < 1.0f) || (frac != 0.0f && k + 1 >= n) || !(cmax >= 1.0f) || !idx ||
                   !ta || !tb))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_stat_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, eps, part,
                       chunks_for(3 * HW / 4), y, idx, ta, tb, (float2*)stat, (int)n, phi, k, frac, cmax, fused);
    VF_RETURN_LAST_ERROR();
}

// out[b] = x_s[k] + frac (x_s[k+1] - x_s[k]), x_s = sort(|x[b][0..n)|): the selection of vf_sample_stat on a plain buffer
int vf_abs_quantile(const float* x, int B, int n, int k, float frac, float* out, void* stream) {
    if (B <= 0) return 0;
    if (n <= 0 || k < 0 || k >= n || !(frac >= 0.0f && frac < 1.0f) || (frac != 0.0f && k + 1 >= n) || !x || !out)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(abs_quantile_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, x, out, n, k, frac);
    VF_RETURN_LAST_ERROR();
}

int vf_p_sample_tail(const float* unet_out, const int* off, const float* y_t, const float* z, const long long* t,
                     const float* sqrt_recip_gammas, const float* sqrt_recipm1_gammas,
                     const float* posterior_log_variance, const float* posterior_mean_coef1,
                     const float* posterior_mean_coef2, float* y_next, float* mean_out, float* weights, int B,
                     int Cout, int HW, int maxV, int weighting, int clip, void* stream) {
    return p_sample_tail<false, false, false>(unet_out, off, nullptr, nullptr, y_t, z, 0, nullptr, t, sqrt_recip_gammas,
                                              sqrt_recipm1_gammas, posterior_log_variance, posterior_mean_coef1,
                                              posterior_mean_coef2, y_next, mean_out, weights, B, Cout, HW, maxV,
                                              weighting, clip, nullptr, 0, 0, stream);
}

int vf_p_sample_tail_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                         const long long* ids, const long long* t, const float* sqrt_recip_gammas,
                         const float* sqrt_recipm1_gammas, const float* posterior_log_variance,
                         const float* posterior_mean_coef1, const float* posterior_mean_coef2, float* y_next,
                         float* mean_out, float* weights, int B, int Cout, int HW, int maxV, int weighting, int clip,
                         void* stream) {
    return p_sample_tail<false, false, true>(unet_out, off, nullptr, nullptr, y_t, nullptr, seed, ids, t,
                                             sqrt_recip_gammas, sqrt_recipm1_gammas, posterior_log_variance,
                                             posterior_mean_coef1, posterior_mean_coef2, y_next, mean_out, weights, B,
                                             Cout, HW, maxV, weighting, clip, nullptr, 0, 0, stream);
}

int vf_p_sample_tail_cfg(const float* unet_out, const int* off, const float* y_t, const float* z, const long long* t,
                         const float* sqrt_recip_gammas, const float* sqrt_recipm1_gammas,
                         const float* posterior_log_variance, const float* posterior_mean_coef1,
                         const float* posterior_mean_coef2, float* y_next, float* mean_out, float* weights, int B,
                         int Cout, int HW, int maxV, int weighting, int clip, const float* g, void* stream) {
    return p_sample_tail<true, false, false>(unet_out, off, nullptr, nullptr, y_t, z, 0, nullptr, t, sqrt_recip_gammas,
                                             sqrt_recipm1_gammas, posterior_log_variance, posterior_mean_coef1,
                                             posterior_mean_coef2, y_next, mean_out, weights, B, Cout, HW, maxV,
                                             weighting, clip, g, 0, 0, stream);
}

int vf_p_sample_tail_cfg_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                             const long long* ids, const long long* t, const float* sqrt_recip_gammas,
                             const float* sqrt_recipm1_gammas, const float* posterior_log_variance,
                             const float* posterior_mean_coef1, const float* posterior_mean_coef2, float* y_next,
                             float* mean_out, float* weights, int B, int Cout, int HW, int maxV, int weighting,
                             int clip, const float* g, void* stream) {
    return p_sample_tail<true, false, true>(unet_out, off, nullptr, nullptr, y_t, nullptr, seed, ids, t,
                                            sqrt_recip_gammas, sqrt_recipm1_gammas, posterior_log_variance,
                                            posterior_mean_coef1, posterior_mean_coef2, y_next, mean_out, weights, B,
                                            Cout, HW, maxV, weighting, clip, g, 0, 0, stream);
}

int vf_p_sample_tail_eps(const float* eps, const float* stat, const float* y_t, const float* z, const long long* t,
                         const float* sqrt_recip_gammas, const float* sqrt_recipm1_gammas,
                         const float* posterior_log_variance, const float* posterior_mean_coef1,
                         const float* posterior_mean_coef2, float* y_next, float* mean_out, int B, int HW, int clip,
                         int rescale, int thr, void* stream) {
    return p_sample_tail<false, true, false>(nullptr, nullptr, eps, stat, y_t, z, 0, nullptr, t, sqrt_recip_gammas,
                                             sqrt_recipm1_gammas, posterior_log_variance, posterior_mean_coef1,
                                             posterior_mean_coef2, y_next, mean_out, nullptr, B, 0, HW, 0, 0, clip,
                                             nullptr, rescale, thr, stream);
}

int vf_p_sample_tail_eps_rng(const float* eps, const float* stat, const float* y_t, unsigned long long seed,
                             const long long* ids, const long long* t, const float* sqrt_recip_gammas,
                             const float* sqrt_recipm1_gammas, const float* posterior_log_variance,
                             const float* posterior_mean_coef1, const float* posterior_mean_coef2, float* y_next,
                             float* mean_out, int B, int HW, int clip, int rescale, int thr, void* stream) {
    return p_sample_tail<false, true, true>(nullptr, nullptr, eps, stat, y_t, nullptr, seed, ids, t, sqrt_recip_gammas,
                                            sqrt_recipm1_gammas, posterior_log_variance, posterior_mean_coef1,
                                            posterior_mean_coef2, y_next, mean_out, nullptr, B, 0, HW, 0, 0, clip,
                                            nullptr, rescale, thr, stream);
}

int vf_sampler_step(const float* unet_out, const int* off, const float* y_t, const float* z, const long long* kidx,
                    const float* a, const float* b, const float* cy, const float* c0, const float* c1,
                    const float* sigma, float* y0_prev, float* y_next, float* weights, int B, int Cout, int HW,
                    int maxV, int weighting, void* stream) {
    return sampler_step<false, false, false>(unet_out, off, nullptr, nullptr, y_t, z, 0, nullptr, kidx, nullptr, a, b,
                                             cy, c0, c1, sigma, y0_prev, y_next, weights, B, Cout, HW, maxV, weighting,
                                             nullptr, 0, 0, stream);
}

int vf_sampler_step_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                        const long long* ids, const long long* kidx, const long long* tau, const float* a,
                        const float* b, const float* cy, const float* c0, const float* c1, const float* sigma,
                        float* y0_prev, float* y_next, float* weights, int B, int Cout, int HW, int maxV,
                        int weighting, void* stream) {
    return sampler_step<false, false, true>(unet_out, off, nullptr, nullptr, y_t, nullptr, seed, ids, kidx, tau, a, b,
                                            cy, c0, c1, sigma, y0_prev, y_next, weights, B, Cout, HW, maxV, weighting,
                                            nullptr, 0, 0, stream);
}

int vf_sampler_step_cfg(const float* unet_out, const int* off, const float* y_t, const float* z,
                        const long long* kidx, const float* a, const float* b, const float* cy, const float* c0,
                        const float* c1, const float* sigma, float* y0_prev, float* y_next, float* weights, int B,
                        int Cout, int HW, int maxV, int weighting, const float* g, void* stream) {
    return sampler_step<true, false, false>(unet_out, off, nullptr, nullptr, y_t, z, 0, nullptr, kidx, nullptr, a, b, cy,
                                            c0, c1, sigma, y0_prev, y_next, weights, B, Cout, HW, maxV, weighting, g, 0,
                                            0, stream);
}

int vf_sampler_step_cfg_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                            const long long* ids, const long long* kidx, const long long* tau, const float* a,
                            const float* b, const float* cy, const float* c0, const float* c1, const float* sigma,
                            float* y0_prev, float* y_next, float* weights, int B, int Cout, int HW, int maxV,
                            int weighting, const float* g, void* stream) {
    return sampler_step<true, false, true>(unet_out, off, nullptr, nullptr, y_t, nullptr, seed, ids, kidx, tau, a, b, cy,
                                           c0, c1, sigma, y0_prev, y_next, weights, B, Cout, HW, maxV, weighting, g, 0,
                                           0, stream);
}

int vf_sampler_step_eps(const float* eps, const float* stat, const float* y_t, const float* z, const long long* kidx,
                        const float* a, const float* b, const float* cy, const float* c0, const float* c1,
                        const float* sigma, float* y0_prev, float* y_next, int B, int HW, int rescale, int thr,
                        void* stream) {
    return sampler_step<false, true, false>(nullptr, nullptr, eps, stat, y_t, z, 0, nullptr, kidx, nullptr, a, b, cy, c0,
                                            c1, sigma, y0_prev, y_next, nullptr, B, 0, HW, 0, 0, nullptr, rescale, thr,
                                            stream);
}

int vf_sampler_step_eps_rng(const float* eps, const float* stat, const float* y_t, unsigned long long seed,
                            const long long* ids, const long long* kidx, const long long* tau, const float* a,
                            const float* b, const float* cy, const float* c0, const float* c1, const float* sigma,
                            float* y0_prev, float* y_next, int B, int HW, int rescale, int thr, void* stream) {
    return sampler_step<false, true, true>(nullptr, nullptr, eps, stat, y_t, nullptr, seed, ids, kidx, tau, a, b, cy, c0,
                                           c1, sigma, y0_prev, y_next, nullptr, B, 0, HW, 0, 0, nullptr, rescale, thr,
                                           stream);
}

// Host mirrors: the same inline functions on the CPU, HOST pointers, no stream (the CPU suite's side of the parity).
int vf_rng_host_philox(const unsigned* counter, const unsigned* key, unsigned* out) {
    vf_philox4x32_10(counter, key, out);
    return 0;
}

int vf_rng_host_normal(unsigned long long seed, const long long* ids, int kind, int step, float* out, int B, int n) {
    if (B < 0 || n < 0 || (n & 3) || !rng_args_ok(kind, step)) return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < n / 4; ++i)
            vf_rng_normal4(seed, (unsigned long long)ids[b], (uint32_t)kind, (uint32_t)step, (uint32_t)i,
                           out + (size_t)b * n + 4 * (size_t)i);
    return 0;
}

int vf_rng_host_train_scalars(unsigned long long seed, const long long* ids, int T, long long* t, float* u, int B) {
    if (B < 0 || T < 2 || T > (1 << 28)) return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b) {
        uint32_t w[4];
        vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
        t[b] = vf_rng_timestep(w[0], T);
        u[b] = vf_rng_uniform24(w[1]);
    }
    return 0;
}

// the training drop draw on the CPU: drop[b] = (word 2 >> 8) < thr for the ids (HOST int64 [B])
int vf_cond_drop_host(unsigned long long seed, const long long* ids, unsigned thr, unsigned char* drop, int B) {
    if (B < 0 || thr > (1u << 24)) return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b) {
        uint32_t w[4];
        vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
        drop[b] = (unsigned char)vf_rng_cond_drop(w[2], thr);
    }
    return 0;
}

// ---- progressive distillation (the head of this file) ----
// i / k1 / k0: DEVICE int64 [B]; level_s [B]; z_t [B][n]; tau_s: DEVICE int64 [K]; exactly one source of i: i_in (DEVICE
// int64 [B], clamped to 0..K-1) or ids (with seed).  n = 3 HW, n % 4 == 0.
int vf_distill_begin(unsigned long long seed, const long long* ids, const long long* i_in, const long long* tau_s,
                     const float* gammas, int K, const float* y_0, const float* noise, long long* i_out, long long* k1,
                     long long* k0, float* level_s, float* z_t, int B, int n, void* stream) {
    if (B <= 0) return 0;
    if (K < 1 || K > (1 << 27) || n <= 0 || (n & 3) || B > 65535) return (int)hipErrorInvalidValue;
    if ((ids == nullptr) == (i_in == nullptr)) return (int)hipErrorInvalidValue;
    if (!tau_s || !gammas || !y_0 || !noise || !i_out || !k1 || !k0 || !level_s || !z_t) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(distill_begin_kernel, dim3(chunks_for(n / 4), B), dim3(256), 0, (hipStream_t)stream, seed, ids, i_in,
                       tau_s, gammas, K, (const float4*)y_0, (const float4*)noise, i_out, k1, k0, level_s, (float4*)z_t,
                       n / 4);
    VF_RETURN_LAST_ERROR();
}

// unet_out [off[B] (+ B with g)][Cout][HW]: the teacher's output at y = z'.  idx = i, kidx = k0: DEVICE int64 [B];
// a / b: the teacher's 2K-entry tables, w1 / w2: the K-entry weights; g (DEVICE fp32 [B] | NULL): guidance scales.
int vf_distill_target(const float* unet_out, const int* off, const float* y, const float* x1, const float* z_t,
                      const float* level_s, const long long* idx, const long long* kidx, const float* a, const float* b,
                      const float* w1, const float* w2, float* x_tilde, float* eps_tilde, int B, int Cout, int HW,
                      int weighting, const float* g, void* stream) {
    if (B <= 0) return 0;
    if (HW <= 0 || (HW & 3) || Cout < 3 || (weighting && Cout < 6) || B > 65535) return (int)hipErrorInvalidValue;
    if (!unet_out || !off || !y || !x1 || !z_t || !level_s || !idx || !kidx || !a || !b || !w1 || !w2 || !x_tilde ||
        !eps_tilde)
        return (int)hipErrorInvalidValue;
    const dim3 grid(chunks_for(3 * HW / 4), B);
    if (g)
        hipLaunchKernelGGL(distill_target_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, unet_out, off, y, x1, z_t,
                           level_s, idx, kidx, a, b, w1, w2, x_tilde, eps_tilde, Cout, HW, weighting, g);
    else
        hipLaunchKernelGGL(distill_target_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, unet_out, off, y, x1, z_t,
                           level_s, idx, kidx, a, b, w1, w2, x_tilde, eps_tilde, Cout, HW, weighting, g);
    VF_RETURN_LAST_ERROR();
}

// Host mirrors.  The seeded draw of i on the CPU: i[b] = mulhi32(word 0, K) for the ids (HOST int64 [B]) ...
int vf_distill_step_host(unsigned long long seed, const long long* ids, int K, long long* i_out, int B) {
    if (B < 0 || K < 1 || K > (1 << 27)) return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b) {
        uint32_t w[4];
        vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
        i_out[b] = vf_rng_distill_step(w[0], K);
    }
    return 0;
}

// ... and vf_loss_weight_pred of the truncated-SNR kind (pred 0 | 1 | 2), which the two mirrors above do not take.
int vf_loss_weights_trunc_snr_host(const float* level, int B, int pred, float* out) {
    if (B < 0 || pred < VF_PRED_EPS || pred > VF_PRED_X0) return (int)hipErrorInvalidValue;
    for (int s = 0; s < B; ++s) out[s] = vf_loss_weight_pred(pred, VF_LOSS_W_TRUNC_SNR, 0.0f, 0.0f, level[s]);
    return 0;
}

// ---- self-conditioning (the head of this file) ----
// vf_stack_views_cfg plus sc (DEVICE [B][3][HW] | NULL: zeros): x [S (+ B)][Cc+6][HW], level_s / angle_s [S (+ B)].
int vf_stack_views_sc(const float* y_cond, const float* y_t, const float* noise, const float* level, const float* angle,
                      const int* off, const unsigned char* drop, const float* sc, float* x, float* level_s,
                      float* angle_s, int B, int Nmax, int Cc, int HW, int S, int copy_cond, int null_rows,
                      void* stream) {
    if (S <= 0 || B <= 0) return 0;
    if ((HW & 3) || Cc < 1 || (null_rows && S < B)) return (int)hipErrorInvalidValue;
    if (!y_t || !level || !angle || !off || !x || !level_s || !angle_s || (copy_cond && !y_cond))
        return (int)hipErrorInvalidValue;
    const int rows = null_rows ? S + B : S;
    if (rows > 65535) return (int)hipErrorInvalidValue;
    const int n4 = 3 * HW / 4, nc4 = Cc * HW / 4;
    hipLaunchKernelGGL(stack_views_cfg_kernel<true>, dim3(chunks_for(nc4 > n4 ? nc4 : n4), rows), dim3(256), 0,
                       (hipStream_t)stream, (const float4*)y_cond, (const float4*)y_t, (const float4*)noise, level, angle,
                       off, drop, (float4*)x, level_s, angle_s, B, Nmax, nc4, n4, copy_cond, S, (const float4*)sc);
    VF_RETURN_LAST_ERROR();
}

int vf_draw_self_cond(unsigned long long seed, const long long* ids, unsigned thr, unsigned char* keep, int B,
                      void* stream) {
    if (B <= 0) return 0;
    if (thr > (1u << 24) || !ids || !keep) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(draw_self_cond_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, seed, ids, thr, keep,
                       B);
    VF_RETURN_LAST_ERROR();
}

// unet_out [off[B]][Cout][HW]: the first pass's output; y_t of sample b at y + row * y_stride + y_off floats, row = off[b]
// (y_by_view != 0: the stacked input, y_stride = (Cc + 6) HW, y_off = Cc HW) or b (a plain [B][3][HW] buffer: 3 HW, 0);
// both multiples of 4; y is not read for pred 2 (x0) and may be NULL there.  keep (DEVICE uint8 [B] | NULL: all kept).
int vf_self_cond_estimate(const float* unet_out, const int* off, const float* level, const float* y, long y_stride,
                          long y_off, int y_by_view, const unsigned char* keep, float* x_hat, int B, int Cout, int HW,
                          int weighting, int pred, void* stream) {
    if (B <= 0) return 0;
    if (HW <= 0 || (HW & 3) || Cout < 3 || (weighting && Cout < 6) || B > 65535) return (int)hipErrorInvalidValue;
    if (pred < VF_PRED_EPS || pred > VF_PRED_X0 || !unet_out || !off || !x_hat) return (int)hipErrorInvalidValue;
    if (pred != VF_PRED_X0 && (!y || !level || y_stride < 3l * HW || y_off < 0 || (y_stride & 3) || (y_off & 3) ||
                               y_off + 3l * HW > y_stride))
        return (int)hipErrorInvalidValue;
    const dim3 grid(chunks_for(3 * HW / 4), B);
    auto kernel = pred == VF_PRED_V ? self_cond_estimate_kernel<VF_PRED_V>
                                    : (pred == VF_PRED_X0 ? self_cond_estimate_kernel<VF_PRED_X0>
                                                          : self_cond_estimate_kernel<VF_PRED_EPS>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, unet_out, off, level, y, (long long)y_stride,
                       (long long)y_off, y_by_view, keep, x_hat, Cout, HW, weighting);
    VF_RETURN_LAST_ERROR();
}

// Host mirrors.  The coin on the CPU: out[b] = (word 3 >> 8) < thr for the ids (HOST int64 [B]) ...
int vf_self_cond_draw_host(unsigned long long seed, const long long* ids, unsigned thr, unsigned char* out, int B) {
    if (B < 0 || thr > (1u << 24)) return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b) {
        uint32_t w[4];
        vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_TRAIN_SCALARS, 0, 0, w);
        out[b] = (unsigned char)vf_rng_self_cond(w[3], thr);
    }
    return 0;
}

// ... and vf_self_cond_coeffs itself: (a, b) of the estimate at levels level [n] for pred 0 | 1 | 2.
int vf_self_cond_coeffs_host(const float* level, int pred, float* a, float* b, int n) {
    if (n < 0 || pred < VF_PRED_EPS || pred > VF_PRED_X0) return (int)hipErrorInvalidValue;
    for (int i = 0; i < n; ++i) vf_self_cond_coeffs(pred, level[i], &a[i], &b[i]);
    return 0;
}

// ---- learned variance (the head of this file; vlb.h) ----
// The hybrid loss: vf_compose_loss_pred_fwd / _bwd for every pred (0 eps: `noise` is the ready-made target and y_0 is not
// read) on a nine-channel unet_out, plus t (DEVICE int64 [B]), the fp32 tables c1, hi, lo [T] and lambda.  var_hat
// [B][3][HW] and vlb_part [B * 64] next to noise_hat and loss_part; sample_vlb [B].  No per-sample scale.  Two launches
// forward, one backward, through loss_fwd / loss_bwd with the LV instantiations.  Refused, as before: what the family's
// launcher of that direction refuses; by both entries (lv_args_ok) Cout < 9, T < 1, HW <= 0, pred outside 0..2, a null
// noise unless x0, a null y_0 unless eps, a null unet_out, off, t, c1, hi, lo or var_hat; by the forward entry also a null
// vlb_part or sample_vlb; by the backward entry also a null level, noise_hat, gloss or dout.  B <= 0 returns 0 first.
static inline bool lv_args_ok(int Cout, int HW, int T, int pred, const float* noise, const float* y_0) {
    if (Cout < 9 || T < 1 || HW <= 0 || pred < VF_PRED_EPS || pred > VF_PRED_X0) return false;
    return (noise || pred == VF_PRED_X0) && (y_0 || pred == VF_PRED_EPS);
}

int vf_compose_loss_lv_fwd(const float* unet_out, const int* off, const float* noise, const float* y_0,
                           const float* level, const long long* t, const float* c1, const float* hi, const float* lo,
                           float* noise_hat, float* var_hat, float* loss_part, float* vlb_part, float* sample_loss,
                           float* sample_w, float* sample_vlb, float* loss, float* bin_sum, int* bin_cnt, int B, int Cout,
                           int HW, int weighting, int penalty, float delta, int weight_kind, float a, float b, int K,
                           int pred, int T, float lambda, void* stream) {
    if (B <= 0) return 0;
    if (!lv_args_ok(Cout, HW, T, pred, noise, y_0) || !unet_out || !off || !t || !c1 || !hi || !lo || !var_hat ||
        !vlb_part || !sample_vlb)
        return (int)hipErrorInvalidValue;
    return loss_fwd<true>(pred, unet_out, off, noise, y_0, level, nullptr, noise_hat, loss_part, sample_loss, sample_w,
                          loss, bin_sum, bin_cnt, B, Cout, HW, weighting, penalty, delta, weight_kind, a, b, K, stream,
                          {VlbArgs{t, c1, hi, lo, T, lambda}, var_hat, vlb_part}, {vlb_part, sample_vlb, lambda});
}

int vf_compose_loss_lv_bwd(const float* unet_out, const int* off, const float* noise, const float* y_0,
                           const float* level, const long long* t, const float* c1, const float* hi, const float* lo,
                           const float* noise_hat, const float* var_hat, const float* gloss, const float* sample_w,
                           float* dout, int B, int Cout, int HW, int weighting, int penalty, float delta, int pred, int T,
                           float lambda, void* stream) {
    if (B <= 0) return 0;
    if (!lv_args_ok(Cout, HW, T, pred, noise, y_0) || !unet_out || !off || !level || !t || !c1 || !hi || !lo ||
        !noise_hat || !var_hat || !gloss || !dout)
        return (int)hipErrorInvalidValue;
    return loss_bwd<true>(pred, unet_out, off, noise, y_0, level, noise_hat, gloss, sample_w, dout, B, Cout, HW,
                          weighting, penalty, delta, stream, {VlbArgs{t, c1, hi, lo, T, lambda}, var_hat});
}

// The learned-variance tail: vf_sampler_step{, _rng, _cfg, _cfg_rng} without c1 and with the tables hi, lo [K] behind
// sigma and lp_out ([B][3][HW] | NULL) behind weights.  unet_out has nine channels.
int vf_sampler_step_lv(const float* unet_out, const int* off, const float* y_t, const float* z, const long long* kidx,
                       const float* a, const float* b, const float* cy, const float* c0, const float* sigma,
                       const float* hi, const float* lo, float* y0_prev, float* y_next, float* weights, float* lp_out,
                       int B, int Cout, int HW, int maxV, int weighting, void* stream) {
    return sampler_step_lv<false, false>(unet_out, off, y_t, z, 0, nullptr, kidx, nullptr, a, b, cy, c0, sigma, hi, lo,
                                         y0_prev, y_next, weights, lp_out, B, Cout, HW, maxV, weighting, nullptr, stream);
}

int vf_sampler_step_lv_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                           const long long* ids, const long long* kidx, const long long* tau, const float* a,
                           const float* b, const float* cy, const float* c0, const float* sigma, const float* hi,
                           const float* lo, float* y0_prev, float* y_next, float* weights, float* lp_out, int B, int Cout,
                           int HW, int maxV, int weighting, void* stream) {
    return sampler_step_lv<false, true>(unet_out, off, y_t, nullptr, seed, ids, kidx, tau, a, b, cy, c0, sigma, hi, lo,
                                        y0_prev, y_next, weights, lp_out, B, Cout, HW, maxV, weighting, nullptr, stream);
}

int vf_sampler_step_lv_cfg(const float* unet_out, const int* off, const float* y_t, const float* z,
                           const long long* kidx, const float* a, const float* b, const float* cy, const float* c0,
                           const float* sigma, const float* hi, const float* lo, float* y0_prev, float* y_next,
                           float* weights, float* lp_out, int B, int Cout, int HW, int maxV, int weighting, const float* g,
                           void* stream) {
    return sampler_step_lv<true, false>(unet_out, off, y_t, z, 0, nullptr, kidx, nullptr, a, b, cy, c0, sigma, hi, lo,
                                        y0_prev, y_next, weights, lp_out, B, Cout, HW, maxV, weighting, g, stream);
}

int vf_sampler_step_lv_cfg_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                               const long long* ids, const long long* kidx, const long long* tau, const float* a,
                               const float* b, const float* cy, const float* c0, const float* sigma, const float* hi,
                               const float* lo, float* y0_prev, float* y_next, float* weights, float* lp_out, int B,
                               int Cout, int HW, int maxV, int weighting, const float* g, void* stream) {
    return sampler_step_lv<true, true>(unet_out, off, y_t, nullptr, seed, ids, kidx, tau, a, b, cy, c0, sigma, hi, lo,
                                       y0_prev, y_next, weights, lp_out, B, Cout, HW, maxV, weighting, g, stream);
}

// Host mirror of vlb.h (HOST pointers, no stream): per element i of n, lp = the log-variance of o[i] between hi[i] and
// lo[i], kl and dkl = KL in bits and dKL/dlp at m^2 = c1[i]^2 kappa^2(level[i]) r[i]^2 for pred 0 | 1 | 2.
int vf_vlb_terms_host(const float* o, const float* hi, const float* lo, const float* c1, const float* level,
                      const float* r, int pred, float* lp, float* kl, float* dkl, int n) {
    if (n < 0 || pred < VF_PRED_EPS || pred > VF_PRED_X0) return (int)hipErrorInvalidValue;
    for (int i = 0; i < n; ++i) {
        const float m2 = vf_vlb_m2(c1[i], vf_vlb_kappa2(pred, level[i]), r[i]);
        lp[i] = vf_vlb_logvar(o[i], hi[i], lo[i]);
        kl[i] = vf_vlb_kl(lp[i], lo[i], m2);
        dkl[i] = vf_vlb_dkl(lp[i], lo[i], m2);
    }
    return 0;
}

// ---- the variational bound (the head of this file; vlb.h) ----
// The noisy targets of step k = kidx[b] (DEVICE int64 [B]) of the chain tau (DEVICE int64 [K]) on the fp32 gammas [T]:
// y_k [B][3][HW] = sqrt(g) y_0 + sqrt(1 - g) n, g = gammas[tau[k]].  noise (DEVICE [B][K][3][HW]) wins; with noise NULL
// n is drawn from (seed, ids[b], kind 6, tau[k], float4 index).  Refused: a null y_0, kidx, tau, gammas or y_k, both noise
// and ids null, HW % 4, HW <= 0, K < 1, T < 1 or T > 2^28.  B <= 0 returns 0 first.
int vf_nll_noisy(const float* y_0, const float* noise, unsigned long long seed, const long long* ids,
                 const long long* kidx, const long long* tau, const float* gammas, float* y_k, int B, int HW, int K,
                 int T, void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || HW <= 0 || K < 1 || T < 1 || T > (1 << 28) || !y_0 || !kidx || !tau || !gammas || !y_k ||
        (!noise && !ids))
        return (int)hipErrorInvalidValue;
    const dim3 grid(chunks_for(3 * HW / 4), B), block(256);
    if (noise)
        hipLaunchKernelGGL(nll_noisy_kernel<false>, grid, block, 0, (hipStream_t)stream, y_0, noise, seed, ids, kidx, tau,
                           gammas, y_k, HW, K, T);
    else
        hipLaunchKernelGGL(nll_noisy_kernel<true>, grid, block, 0, (hipStream_t)stream, y_0, noise, seed, ids, kidx, tau,
                           gammas, y_k, HW, K, T);
    VF_RETURN_LAST_ERROR();
}

// One term of the bound for every sample, at step k = kidx[b] (DEVICE int64 [B], clamped into [0, K - 1]) of the fp32
// tables a, b, c0, hi, lo [K] (schedule.nll_tables): vb [B][K] and x0_mse [B][K] receive column k -- the mean over the
// sample's 3 HW elements of the term in bits and of (y0 - y_0)^2.  lv: unet_out has nine channels and lp lies between
// lo[k] and hi[k] by the composed channels 6..8; else lp = hi[k] where `large`, lo[k] otherwise.  dec: the decoder
// likelihood instead of the KL (the caller's k == 0).  clip: y0 is clamped to [-1, 1].  vb_part, sq_part: [B * 64]
// scratch.  Two launches, no atomics.  Refused: a null pointer, HW % 4, HW <= 0, K < 1, Cout < 3 (6 with weighting, 9
// with lv), lv together with large.  B <= 0 returns 0 first.
int vf_nll_terms(const float* unet_out, const int* off, const float* y_k, const float* y_0, const long long* kidx,
                 const float* a, const float* b, const float* c0, const float* hi, const float* lo, float* vb_part,
                 float* sq_part, float* vb, float* x0_mse, int B, int Cout, int HW, int K, int weighting, int clip, int lv,
                 int dec, int large, void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || HW <= 0 || K < 1 || Cout < (lv ? 9 : (weighting ? 6 : 3)) || (lv && large))
        return (int)hipErrorInvalidValue;
    if (!unet_out || !off || !y_k || !y_0 || !kidx || !a || !b || !c0 || !hi || !lo || !vb_part || !sq_part || !vb ||
        !x0_mse)
        return (int)hipErrorInvalidValue;
    const int ch = chunks_for(3 * HW / 4);
    auto kern = lv ? (dec ? nll_term_kernel<true, true> : nll_term_kernel<true, false>)
                   : (dec ? nll_term_kernel<false, true> : nll_term_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3(ch, B), dim3(256), 0, (hipStream_t)stream, unet_out, off, y_k, y_0, kidx, a, b, c0, hi,
                       lo, vb_part, sq_part, Cout, HW, K, weighting, clip, large);
    hipLaunchKernelGGL(nll_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                       (const float*)vb_part, (const float*)sq_part, kidx, vb, x0_mse, B, ch, K,
                       1.0f / (float)(3 * HW));
    VF_RETURN_LAST_ERROR();
}

// The prior term L_T of every sample, prior [B] in bits per dimension, from y_0 and gammas[T - 1]; part: [B * 64] scratch.
// Refused: a null pointer, HW % 4, HW <= 0, T < 1.  B <= 0 returns 0 first.
int vf_nll_prior(const float* y_0, const float* gammas, float* part, float* prior, int B, int HW, int T, void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || HW <= 0 || T < 1 || !y_0 || !gammas || !part || !prior) return (int)hipErrorInvalidValue;
    const int ch = chunks_for(3 * HW / 4);
    hipLaunchKernelGGL(nll_prior_kernel, dim3(ch, B), dim3(256), 0, (hipStream_t)stream, y_0, gammas, part, HW, T);
    hipLaunchKernelGGL(nll_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const float*)part,
                       (const float*)nullptr, (const long long*)nullptr, prior, (float*)nullptr, B, ch, 1,
                       1.0f / (float)(3 * HW));
    VF_RETURN_LAST_ERROR();
}

// Host mirror of one term (HOST pointers, no stream): element i of n has its own composed prediction out[i], raw variance
// o[i] (read with lv alone; NULL otherwise), y_k[i], y_0[i] and table row (a, b, c0, hi, lo)[i]; term[i] in bits and
// sq[i] = (y0 - y_0)^2 by the very function the kernel runs.  Refused: n < 0, lv together with large, and with n > 0 a null
// pointer (o only with lv).
int vf_nll_terms_host(const float* out, const float* o, const float* y_k, const float* y_0, const float* a,
                      const float* b, const float* c0, const float* hi, const float* lo, int lv, int dec, int large,
                      int clip, float* term, float* sq, int n) {
    if (n < 0 || (lv && large)) return (int)hipErrorInvalidValue;
    if (n > 0 && (!out || (lv && !o) || !y_k || !y_0 || !a || !b || !c0 || !hi || !lo || !term || !sq))
        return (int)hipErrorInvalidValue;
    for (int i = 0; i < n; ++i) {
        const NllRow row{a[i], b[i], c0[i], hi[i], lo[i]};
        const float lp = lv ? vf_vlb_logvar(o[i], row.hi, row.lo) : (large ? row.hi : row.lo);
        term[i] = dec ? nll_element<true>(row, out[i], lp, y_k[i], y_0[i], clip, &sq[i])
                      : nll_element<false>(row, out[i], lp, y_k[i], y_0[i], clip, &sq[i]);
    }
    return 0;
}

// ---- the analytic variance (the head of this file) ----
// The second moment of the noise estimate of every sample at step k = kidx[b] (DEVICE int64 [B], clamped into
// [0, K - 1]) of the fp32 tables ea, eb [K] (schedule.eps_tables): m2 [B][K] receives column k -- the mean over the
// sample's 3 HW elements of (ea[k] y_k + eb[k] out_b)^2, out_b the composition of channels 0..2 over the sample's views.
// part: [B * 64] scratch.  Two launches (the second is the bound's finish kernel), no atomics.  Refused: a null pointer,
// HW % 4, HW <= 0, K < 1, Cout < 3 (6 with weighting).  B <= 0 returns 0 first.
int vf_eps_moments(const float* unet_out, const int* off, const float* y_k, const long long* kidx, const float* ea,
                   const float* eb, float* part, float* m2, int B, int Cout, int HW, int K, int weighting,
                   void* stream) {
    if (B <= 0) return 0;
    if ((HW & 3) || HW <= 0 || K < 1 || Cout < (weighting ? 6 : 3)) return (int)hipErrorInvalidValue;
    if (!unet_out || !off || !y_k || !kidx || !ea || !eb || !part || !m2) return (int)hipErrorInvalidValue;
    const int ch = chunks_for(3 * HW / 4);
    hipLaunchKernelGGL(eps_moment_kernel, dim3(ch, B), dim3(256), 0, (hipStream_t)stream, unet_out, off, y_k, kidx, ea,
                       eb, part, Cout, HW, K, weighting);
    hipLaunchKernelGGL(nll_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const float*)part,
                       (const float*)nullptr, kidx, m2, (float*)nullptr, B, ch, K, 1.0f / (float)(3 * HW));
    VF_RETURN_LAST_ERROR();
}

// Host mirror of one element of the moment (HOST pointers, no stream): element i of n has its own composed prediction
// out[i], y_k[i] and table row (ea, eb)[i]; eps[i] = the noise estimate and sq[i] = its square, by the very function the
// kernel runs.  Refused: n < 0, and with n > 0 a null pointer.
int vf_eps_moment_host(const float* out, const float* y_k, const float* ea, const float* eb, float* eps, float* sq,
                       int n) {
    if (n < 0) return (int)hipErrorInvalidValue;
    if (n > 0 && (!out || !y_k || !ea || !eb || !eps || !sq)) return (int)hipErrorInvalidValue;
    for (int i = 0; i < n; ++i) sq[i] = eps_moment_element(ea[i], eb[i], out[i], y_k[i], &eps[i]);
    return 0;
}

}  // extern "C"
