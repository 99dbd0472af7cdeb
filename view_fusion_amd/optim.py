"""Adam for the ViewFusion training step as ONE multi-tensor HIP launch.

Drop-in for `torch.optim.Adam(params, lr)` as the reference uses it (experiment.py:118-120: default
betas/eps, no weight decay, no amsgrad); `state_dict()` uses torch's keys (`step`, `exp_avg`,
`exp_avg_sq`) so optimizer checkpoints interchange.  The learning rate is read from
`param_group["lr"]` every step (the reference sets it from its LrScheduler before each step).

Step counts are per parameter, as in torch: the parameters of a group that share a step count form one
"bucket" = one launch (in the ViewFusion UNet every parameter receives a gradient every iteration, so
there is exactly one bucket); a parameter that joins later (first gradient at iteration k) gets a bucket
of its own with its own bias corrections.

Two opt-in extras ride the same launch (both off by default: the step is then exactly the launch described above):

  * `max_grad_norm`: global-norm gradient clipping, `torch.nn.utils.clip_grad_norm_`'s arithmetic.  Two extra launches
    take the L2 norm of ALL gradients of the step (per-block partial sums in double, one workgroup adds them in a fixed
    order: no atomics, bit-reproducible) and leave {norm, scale = min(1, max_norm / (norm + 1e-6))} in device memory; the
    update reads g * scale.  The STORED gradients are not scaled: `p.grad` after a step is the raw gradient.
    `grad_norm` is a 0-d device tensor with the last step's pre-clip norm (reading it is the caller's sync, the step has
    none).  `max_grad_norm=float("inf")` measures the norm without ever clipping (scale == 1: bit-identical updates).
  * `ema_decay`: an exponential moving average of the weights, ema = fma(d, ema, (1 - d) p_new) per element in the same
    launch (csrc/adam_update.h states the rounding).  The EMA tensors start as copies of the parameters at a
    parameter's first step; with `ema_warmup` the decay of the update number t (0 for the first) is
    min(ema_decay, (1 + t) / (10 + t)).  `ema_state_dict()` / `load_ema_state_dict()` keep them OUTSIDE `state_dict()`,
    which stays torch's.  `swap_ema()` exchanges parameters and EMA in place (see train.Trainer.ema_weights).

Gradient accumulation (opt-in, for a step whose batch runs as several micro-batches; train.Trainer(accum_steps=)):
`accumulate(weight, first)` after each micro-batch's backward adds weight * p.grad into one accumulator per parameter in
ONE launch (acc = w g on the first micro-batch, which never reads the accumulator, acc + w g afterwards; csrc/adam_update.h
states the rounding; no atomics); the next `step()` takes the accumulators as its gradients -- for the norm pass, the
update and `grad_norm` alike -- and leaves them in `p.grad`.  A `step()` without an `accumulate()` before it is the step
described above, launch for launch.  One accumulator set per optimizer, the size of the parameters.
"""
import ctypes

import torch

from . import _lib, ops


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, ema_decay=None, ema_warmup=False,
                 max_grad_norm=None):
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay}")
        if ema_warmup and ema_decay is None:
            raise ValueError("ema_warmup needs ema_decay")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._plans = {}          # per param group: buckets of {descriptor rows, staging buffers, step count}
        self.graph_epoch = 0      # bumped whenever the state tensors a captured step addresses are replaced
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self._max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._ema = {}            # parameter -> its EMA tensor (kept out of self.state: state_dict() stays torch's)
        self._ema_t = 0           # EMA updates so far
        self._xs = None           # device float[8]: {d, 1 - d, max_norm, norm, scale, -, -, -}
        self._partials = None     # device double[blocks]: the norm pass' per-block sums
        self._swap = None         # swap_ema()'s descriptor table
        self._acc = {}            # parameter -> its gradient accumulator (accumulate())
        self._acc_plan = None     # accumulate()'s descriptor table {acc, grad, -, -, numel, first_block}
        self._acc_scal = None     # device float[4]: {beta, w, -, -} of the coming accumulate launch
        self._acc_live = False    # accumulate() ran since the last step(): step() reads the accumulators

    # -- the opt-in extras: weight EMA, global-norm clipping ------------------------------------------------------------
    @property
    def _extras(self):
        return self.ema_decay is not None or self.max_grad_norm is not None

    def _xs_buf(self, dev):
        if self._xs is None or self._xs.device != dev:
            self._xs = torch.zeros(8, device=dev, dtype=torch.float32)
        return self._xs

    def _xs_ptr(self, i):
        return ctypes.c_void_p(self._xs.data_ptr() + 4 * i)

    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        """The VALUE may change at any time (the kernels read it from device memory, a captured step included); whether
        the norm launches exist at all is fixed at construction, and with it what a captured step contains."""
        if (value is None) != (self._max_grad_norm is None):
            raise ValueError("max_grad_norm cannot be switched on or off after construction (the norm launches are part "
                             "of the step a graph captured); pass float('inf') to measure the norm without clipping")
        if value is not None and not float(value) > 0.0:
            raise ValueError(f"max_grad_norm must be positive, got {value}")
        self._max_grad_norm = None if value is None else float(value)

    @property
    def grad_norm(self):
        """0-d device tensor: the global L2 norm of the last step's gradients before clipping (a view of memory the
        norm pass writes: it follows every step, captured ones included).  None without max_grad_norm."""
        if self.max_grad_norm is None:
            return None
        for group in self.param_groups:
            for p in group["params"]:
                if p.is_cuda:
                    return self._xs_buf(p.device)[3]
        return None

    def _ema_scalars(self):
        """(d, 1 - d) of the coming EMA update, in double."""
        if self.ema_decay is None:
            return 0.0, 0.0
        d = self.ema_decay
        if self.ema_warmup:
            d = min(d, (1.0 + self._ema_t) / (10.0 + self._ema_t))
        return d, 1.0 - d

    def _ema_of(self, p):
        e = self._ema.get(p)
        if e is None:
            e = self._ema[p] = p.detach().clone(memory_format=torch.contiguous_format)
        return e

    def _all_params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def ema_state_dict(self):
        """{"num_updates": EMA updates so far, "state": {index: EMA tensor}} with the index = the parameter's position
        over all groups, like torch's optimizer state.  The tensors are the live ones, not copies (as in torch's
        state_dict()): between two swap_ema() calls -- inside train.Trainer.ema_weights() -- they hold the LIVE weights."""
        return dict(num_updates=self._ema_t,
                    state={i: self._ema[p] for i, p in enumerate(self._all_params()) if p in self._ema})

    @torch.no_grad()
    def load_ema_state_dict(self, sd):
        if self.ema_decay is None:
            raise _lib.VFHipError("load_ema_state_dict: this optimizer was built without ema_decay")
        params, created = self._all_params(), False
        for i, t in sd["state"].items():
            p = params[int(i)]
            if tuple(t.shape) != tuple(p.shape):
                raise _lib.VFHipError(f"load_ema_state_dict: entry {i} has shape {tuple(t.shape)}, the parameter "
                                      f"{tuple(p.shape)}")
            if p in self._ema:                        # in place: captured steps keep addressing this tensor
                self._ema[p].copy_(t)
            else:
                self._ema[p] = t.detach().to(device=p.device, dtype=torch.float32, copy=True).contiguous()
                created = True
        self._ema_t = int(sd["num_updates"])
        if created:
            for gi in self._plans:
                self._flush_steps(gi)
            self._plans = {}
            self.graph_epoch += 1

    @torch.no_grad()
    def swap_ema(self):
        """Exchange parameters and EMA IN PLACE, one launch: the contents move, every address stays (captured graphs and
        the packed-weight caches address parameter memory by raw pointer; the version counters are bumped so the packs
        refresh).  Calling it twice restores both bit for bit."""
        if self.ema_decay is None:
            raise _lib.VFHipError("swap_ema: this optimizer was built without ema_decay")
        params = self._all_params()
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.VFHipError("FusedAdam needs contiguous float32 GPU parameters")
        key = tuple((p.data_ptr(), self._ema_of(p).data_ptr()) for p in params)
        sw = self._swap
        if sw is None or sw["key"] != key:
            rows, first = [], 0
            for p in params:
                rows.append([p.data_ptr(), 0, 0, 0, p.numel(), first])
                first += (p.numel() + 1023) // 1024
            dev = params[0].device
            sw = self._swap = dict(key=key, blocks=first, numel=sum(p.numel() for p in params),
                                   dev=torch.tensor(rows, dtype=torch.int64).to(dev),
                                   ema=torch.tensor([e for _, e in key], dtype=torch.int64).to(dev))
        ops._launch("adam", 0.0, "vf_swap_multi", ctypes.c_void_p(sw["dev"].data_ptr()),
                    ctypes.c_void_p(sw["ema"].data_ptr()), len(params), sw["blocks"],
                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), nbytes=16.0 * sw["numel"])
        torch.autograd.graph.increment_version(params)

    # -- descriptor tables ---------------------------------------------------------------------------------------
    def _flush_steps(self, gi):
        """Write the buckets' step counters back into the per-parameter state (torch's `step` entries)."""
        for b in self._plans.get(gi, {}).get("buckets", ()):
            for p in b["params"]:
                self.state[p]["step"] = torch.tensor(float(b["t"]))
        ext = getattr(self, "_ext", None)
        if ext is not None and gi == 0 and ext["epoch"] == self.graph_epoch:
            for p in ext["params"]:
                self.state[p]["step"] = torch.tensor(float(ext["t"]))

    # -- an exchange step that applies the update itself (reducer.XgmiArena: all-reduce fused with Adam) -----------
    def external_begin(self):
        """One iteration of a reducer that runs this optimizer's update inside its own kernels: state for EVERY
        parameter (created if missing), one common step count, advanced by one here.  Returns (handle, (lr, 1-b1^t,
        1-b2^t, b1, b2, eps)); the caller's kernels update p / exp_avg / exp_avg_sq in place (adam.hip's arithmetic), so
        `state_dict()` stays torch's and a later plain `step()` continues from the same counters."""
        if self._extras:
            raise _lib.VFHipError("FusedAdam.external_begin: ema_decay / max_grad_norm are not part of an external "
                                  "reducer's fused update (the xgmi all-reduce + Adam kernel); leave both off there")
        if len(self.param_groups) != 1:
            raise _lib.VFHipError("FusedAdam.external_begin: one parameter group")
        group = self.param_groups[0]
        ext = getattr(self, "_ext", None)
        if ext is None or ext["epoch"] != self.graph_epoch:
            for gi in self._plans:
                self._flush_steps(gi)
            steps = set()
            for p in group["params"]:
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise _lib.VFHipError("FusedAdam needs contiguous float32 GPU parameters")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                steps.add(int(float(st["step"])))
            if len(steps) != 1:
                raise _lib.VFHipError("FusedAdam.external_begin: the parameters carry different step counts")
            self._plans = {}                               # (a later plain step() re-reads the counters from the state)
            ext = self._ext = dict(params=list(group["params"]), t=steps.pop(), epoch=self.graph_epoch)
        ext["t"] += 1
        b1, b2 = group["betas"]
        t = ext["t"]
        return ext, (float(group["lr"]), 1.0 - b1 ** t, 1.0 - b2 ** t, float(b1), float(b2), float(group["eps"]))

    def _plan(self, gi, group):
        """Static part of the descriptor tables {param, grad, exp_avg, exp_avg_sq, numel, first_block}: built once
        (state tensors never move); only the gradient pointers can change from step to step."""
        params = [p for p in group["params"] if p.grad is not None]
        key = tuple(id(p) for p in params)
        plan = self._plans.get(gi)
        if plan is not None and plan["key"] == key:
            return plan
        self._flush_steps(gi)                          # a changed parameter set must not restart the bias correction
        self._ext = None                               # (an external reducer's counters have just been flushed)
        self.graph_epoch += 1
        by_step = {}
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.VFHipError("FusedAdam needs contiguous float32 GPU parameters")
            st = self.state[p]
            if not st:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p)
                st["exp_avg_sq"] = torch.zeros_like(p)
            by_step.setdefault(int(float(st["step"])), []).append(p)
        buckets = []
        for t, ps in sorted(by_step.items()):
            rows, first = [], 0
            for p in ps:
                st = self.state[p]
                rows.append([p.data_ptr(), 0, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), first])
                first += (p.numel() + 1023) // 1024
            dev = ps[0].device
            buckets.append(dict(params=ps, blocks=first, t=t, numel=sum(p.numel() for p in ps),
                                host=[torch.tensor(rows, dtype=torch.int64).pin_memory() for _ in range(2)],
                                dev=[torch.empty(len(rows), 6, dtype=torch.int64, device=dev) for _ in range(2)],
                                ptrs=[None, None], done=[None, None], flip=0))
            if self.ema_decay is not None:             # one EMA pointer per descriptor row (a table of its own: the
                # row layout above is shared with csrc/xgmi.hip); EMA tensors are born as copies of the parameters
                buckets[-1]["ema_dev"] = torch.tensor([self._ema_of(p).data_ptr() for p in ps], dtype=torch.int64).to(dev)
        plan = dict(key=key, buckets=buckets)
        self._plans[gi] = plan
        return plan

    def state_dict(self):
        for gi in set(self._plans) | {0}:              # the per-parameter step counters are kept lazily
            self._flush_steps(gi)
        return super().state_dict()

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self._plans = {}
        self.graph_epoch += 1                          # new exp_avg / exp_avg_sq tensors: captured steps are stale

    # -- HIP-graph capture of a whole training step (train.Trainer) ------------------------------------------------
    # A captured step cannot carry step-dependent launch arguments, so the update reads {lr, 1-b1^t, 1-b2^t} from three
    # device floats that `graph_tick` refreshes (as launch arguments of a one-thread kernel) before every replay.
    def graph_begin(self):
        """Handle for capturing `step_captured`, or None when the update is not ONE launch over ALL parameters (more
        than one group or bucket, a parameter without state yet): the caller then stays on the eager path."""
        if len(self.param_groups) != 1:
            return None
        plan = self._plans.get(0)
        if plan is None or len(plan["buckets"]) != 1:
            return None
        b = plan["buckets"][0]
        if len(b["params"]) != len(self.param_groups[0]["params"]):
            return None
        rows = b["host"][0].clone()
        h = dict(bucket=b, rows=rows, epoch=self.graph_epoch, dev=torch.empty(rows.shape, dtype=torch.int64, device=b["params"][0].device))
        if self._extras:                               # what the extra launches of the captured step address
            dev = b["params"][0].device
            h["xs"] = self._xs_buf(dev)
            if self.max_grad_norm is not None:
                h["partials"] = torch.empty(b["blocks"], dtype=torch.float64, device=dev)
        return h

    @torch.no_grad()
    def step_captured(self, h, scalars):
        """Inside the capture, after backward(): the one multi-tensor launch.  The descriptor table's contents (the
        gradient addresses this capture allocated) are uploaded by `graph_end` once the capture has ended."""
        b, group = h["bucket"], self.param_groups[0]
        b1, b2 = group["betas"]
        if self._extras:
            raw = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            desc, n, clip, ema = ctypes.c_void_p(h["dev"].data_ptr()), len(b["params"]), "partials" in h, "ema_dev" in b
            if clip:
                part = ctypes.c_void_p(h["partials"].data_ptr())
                _lib.call("vf_grad_sumsq_multi", desc, n, b["blocks"], part, raw)
                _lib.call("vf_grad_norm_finish", part, b["blocks"], self._xs_ptr(2), self._xs_ptr(3), raw)
            _lib.call("vf_adam_multi_ex_dev", desc, ctypes.c_void_p(b["ema_dev"].data_ptr()) if ema else None, n,
                      b["blocks"], ctypes.c_void_p(scalars.data_ptr()), float(b1), float(b2), float(group["eps"]),
                      self._xs_ptr(4) if clip else None, self._xs_ptr(0) if ema else None, raw)
            return
        _lib.call("vf_adam_multi_dev", ctypes.c_void_p(h["dev"].data_ptr()), len(b["params"]), b["blocks"],
                  ctypes.c_void_p(scalars.data_ptr()), float(b1), float(b2), float(group["eps"]),
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def graph_end(self, h):
        grads = [p.grad for p in h["bucket"]["params"]]
        if any(g is None or not g.is_contiguous() for g in grads):
            raise _lib.VFHipError("captured training step: a parameter received no (or a strided) gradient")
        h["rows"][:, 1] = torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64)
        h["dev"].copy_(h["rows"])
        h["grads"] = grads                             # the graph writes these allocations on every replay
        return h

    def graph_tick(self, h, scalars):
        """Before a replay: advance the step count and hand the replay its learning rate and bias corrections."""
        b, group = h["bucket"], self.param_groups[0]
        b["t"] += 1
        b1, b2 = group["betas"]
        if self._extras:
            d, omd = self._ema_scalars()
            _lib.call("vf_adam_set_scalars_ex", ctypes.c_void_p(scalars.data_ptr()), float(group["lr"]),
                      1.0 - b1 ** b["t"], 1.0 - b2 ** b["t"], self._xs_ptr(0), d, omd, self.max_grad_norm or 0.0,
                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            if self.ema_decay is not None:
                self._ema_t += 1
        else:
            _lib.call("vf_adam_set_scalars", ctypes.c_void_p(scalars.data_ptr()), float(group["lr"]), 1.0 - b1 ** b["t"],
                      1.0 - b2 ** b["t"], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.autograd.graph.increment_version(b["params"])

    # -- gradient accumulation over micro-batches ------------------------------------------------------------------
    def _accum_plan(self, first):
        """Descriptor table of accumulate(): rows {accumulator, gradient, -, -, numel, first_block} over every parameter
        that has a gradient; the accumulators are made once per parameter and never move."""
        params = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        key = tuple(id(p) for p in params)
        a = self._acc_plan
        if a is not None and a["key"] == key:
            return a
        if not first:
            raise _lib.VFHipError("FusedAdam.accumulate: the set of parameters with a gradient changed between the "
                                  "micro-batches of one step")
        if not params:
            raise _lib.VFHipError("FusedAdam.accumulate: no parameter has a gradient")
        rows, first_block = [], 0
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.VFHipError("FusedAdam needs contiguous float32 GPU parameters")
            if p not in self._acc:                     # (never read before the first accumulate has written it)
                self._acc[p] = torch.empty_like(p, memory_format=torch.contiguous_format)
            rows.append([self._acc[p].data_ptr(), 0, 0, 0, p.numel(), first_block])
            first_block += (p.numel() + 1023) // 1024
        dev = params[0].device
        if self._acc_scal is None or self._acc_scal.device != dev:
            self._acc_scal = torch.zeros(4, device=dev, dtype=torch.float32)
        a = self._acc_plan = dict(key=key, params=params, blocks=first_block, numel=sum(p.numel() for p in params),
                                  host=[torch.tensor(rows, dtype=torch.int64).pin_memory() for _ in range(2)],
                                  dev=[torch.empty(len(rows), 6, dtype=torch.int64, device=dev) for _ in range(2)],
                                  ptrs=[None, None], done=[None, None], flip=0)
        return a

    def _accum_scalars(self, weight, first, raw):
        ops._launch("adam", 0.0, "vf_adam_set_scalars", ctypes.c_void_p(self._acc_scal.data_ptr()),
                    0.0 if first else 1.0, float(weight), 0.0, raw)

    @torch.no_grad()
    def accumulate(self, weight, first):
        """After a micro-batch's backward: acc = (0 if first else acc) + weight * p.grad for every parameter with a
        gradient, one launch (plus the one-thread launch that hands it {beta, weight}); the next step() uses the
        accumulators as its gradients.  `first` starts a new sum: the accumulators are overwritten, never read."""
        stream = torch.cuda.current_stream()
        raw = ctypes.c_void_p(stream.cuda_stream)
        a = self._accum_plan(first)
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in a["params"]]
        f = self._table_with(a, [g.data_ptr() for g in grads], stream)
        self._accum_scalars(weight, first, raw)
        ops._launch("adam", 0.0, "vf_grad_accum_multi", ctypes.c_void_p(a["dev"][f].data_ptr()), len(grads), a["blocks"],
                    ctypes.c_void_p(self._acc_scal.data_ptr()), raw, nbytes=(8.0 if first else 12.0) * a["numel"])
        self._acc_live = True

    # the capturable form (train.Trainer: forward + backward + the accumulate launch as one graph per micro-batch
    # geometry): the launch reads {beta, weight} from device memory that `accum_tick` refreshes before every replay
    def accum_begin(self):
        """Handle for capturing `accumulate_captured`, or None before the first eager accumulate() (no accumulators
        yet) or when it did not cover every parameter."""
        a = self._acc_plan
        if a is None or len(a["params"]) != sum(len(g["params"]) for g in self.param_groups):
            return None
        rows = a["host"][0].clone()
        return dict(plan=a, rows=rows, dev=torch.empty(rows.shape, dtype=torch.int64, device=a["params"][0].device))

    @torch.no_grad()
    def accumulate_captured(self, h):
        """Inside the capture, after backward(): the accumulate launch on the gradients this capture allocated (their
        addresses reach the table in `accum_end`, once the capture has ended)."""
        a = h["plan"]
        _lib.call("vf_grad_accum_multi", ctypes.c_void_p(h["dev"].data_ptr()), len(a["params"]), a["blocks"],
                  ctypes.c_void_p(self._acc_scal.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def accum_end(self, h):
        grads = [p.grad for p in h["plan"]["params"]]
        if any(g is None or not g.is_contiguous() for g in grads):
            raise _lib.VFHipError("captured micro-batch: a parameter received no (or a strided) gradient")
        h["rows"][:, 1] = torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64)
        h["dev"].copy_(h["rows"])
        h["grads"] = grads                             # the graph writes these allocations on every replay
        return h

    def accum_tick(self, h, weight, first):
        """Before a replay: this micro-batch's {beta, weight}."""
        if h["plan"] is not self._acc_plan:
            raise _lib.VFHipError("FusedAdam.accum_tick: the accumulators changed since this micro-batch was captured")
        _lib.call("vf_adam_set_scalars", ctypes.c_void_p(self._acc_scal.data_ptr()), 0.0 if first else 1.0, float(weight),
                  0.0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        self._acc_live = True

    # -- the step ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        stream = torch.cuda.current_stream()
        raw = ctypes.c_void_p(stream.cuda_stream)
        if self._acc_live:                             # the accumulated gradient is this step's gradient, and what
            for p in self._acc_plan["params"]:         # p.grad shows after it (stable addresses: the tables below are
                p.grad = self._acc[p]                  # uploaded once)
            self._acc_live = False
        if self._extras:
            self._step_extras(stream, raw)
            return loss
        for gi, group in enumerate(self.param_groups):
            if not any(p.grad is not None for p in group["params"]):
                continue
            b1, b2 = group["betas"]
            for b in self._plan(gi, group)["buckets"]:
                b["t"] += 1
                t = b["t"]
                f, grads = self._grad_table(b, stream)    # (grads: a .contiguous() copy lives until the launch is enqueued)
                ops._launch("adam", 0.0, "vf_adam_multi", ctypes.c_void_p(b["dev"][f].data_ptr()), len(grads), b["blocks"],
                            float(group["lr"]), float(b1), float(b2), float(group["eps"]), 1.0 - b1 ** t, 1.0 - b2 ** t,
                            raw, nbytes=28.0 * b["numel"])   # 4 reads + 3 writes
                # the kernel writes through raw pointers: tell autograd (and the packed-weight caches of ops/packing.py,
                # which are keyed on the version counter) that the parameters changed
                torch.autograd.graph.increment_version(b["params"])
        return loss

    def _grad_table(self, b, stream):
        """Bucket b's descriptor table with this step's gradient addresses -> (which of its two copies, the gradient
        tensors the table points at: the caller keeps them until every launch that reads the table is enqueued)."""
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in b["params"]]
        return self._table_with(b, [g.data_ptr() for g in grads], stream), grads

    @staticmethod
    def _table_with(b, ptrs, stream):
        """Which of table b's two device copies holds the gradient addresses `ptrs` (uploaded if neither does)."""
        f = b["flip"]
        if b["ptrs"][f] != ptrs:               # gradient arena / stable allocations: the table is reused as is
            f = b["flip"] = f ^ 1
            if b["ptrs"][f] != ptrs:
                # two staging buffers, each guarded by an event: the H2D copy that last read this pinned
                # buffer (two steps ago) must have executed before the host overwrites it -- the host may
                # run several iterations ahead of the GPU
                if b["done"][f] is not None:
                    b["done"][f].synchronize()
                b["host"][f][:, 1] = torch.tensor(ptrs, dtype=torch.int64)
                b["dev"][f].copy_(b["host"][f], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(stream)
                b["done"][f], b["ptrs"][f] = ev, ptrs
        return f

    def _step_extras(self, stream, raw):
        """step() with max_grad_norm and / or ema_decay: the norm over ALL gradients of the step first (every group and
        bucket), then one update launch per bucket that reads the scale and carries the EMA."""
        work = []
        for gi, group in enumerate(self.param_groups):
            if not any(p.grad is not None for p in group["params"]):
                continue
            for b in self._plan(gi, group)["buckets"]:
                b["t"] += 1
                work.append((group, b) + self._grad_table(b, stream))
        if not work:
            return
        dev = work[0][1]["params"][0].device
        self._xs_buf(dev)
        clip = self.max_grad_norm is not None
        d, omd = self._ema_scalars()
        ops._launch("adam", 0.0, "vf_adam_set_scalars_ex", None, 0.0, 0.0, 0.0, self._xs_ptr(0), d, omd,
                    self.max_grad_norm or 0.0, raw)
        if clip:
            total = sum(w[1]["blocks"] for w in work)
            if self._partials is None or self._partials.numel() < total or self._partials.device != dev:
                self._partials = torch.empty(total, dtype=torch.float64, device=dev)
            off = 0
            for _, b, f, grads in work:
                ops._launch("adam", 0.0, "vf_grad_sumsq_multi", ctypes.c_void_p(b["dev"][f].data_ptr()), len(grads), b["blocks"],
                            ctypes.c_void_p(self._partials.data_ptr() + 8 * off), raw, nbytes=4.0 * b["numel"])
                off += b["blocks"]
            ops._launch("adam", 0.0, "vf_grad_norm_finish", ctypes.c_void_p(self._partials.data_ptr()), total,
                        self._xs_ptr(2), self._xs_ptr(3), raw, nbytes=8.0 * total)
        for group, b, f, grads in work:           # (work keeps every bucket's gradient tensors alive up to here)
            b1, b2 = group["betas"]
            t, n = b["t"], len(grads)
            ema = b.get("ema_dev")
            ops._launch("adam", 0.0, "vf_adam_multi_ex", ctypes.c_void_p(b["dev"][f].data_ptr()),
                        None if ema is None else ctypes.c_void_p(ema.data_ptr()), n, b["blocks"], float(group["lr"]),
                        float(b1), float(b2), float(group["eps"]), 1.0 - b1 ** t, 1.0 - b2 ** t,
                        self._xs_ptr(4) if clip else None, None if ema is None else self._xs_ptr(0), raw,
                        nbytes=(28.0 if ema is None else 36.0) * b["numel"])
            torch.autograd.graph.increment_version(b["params"])
        if self.ema_decay is not None:
            self._ema_t += 1
