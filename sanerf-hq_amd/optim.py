"""Adam with the update of each parameter tensor as ONE HIP kernel (csrc/optim.hip: sn_adam_step) -- or, with `multi_tensor=True`, of
every parameter tensor of the model in ONE launch (sn_adam_step_multi).

Drop-in for the optimiser the reference constructs (main.py:283: `torch.optim.Adam(model.get_params(lr), eps=1e-15)`):
same constructor arguments, same `state_dict` layout (`step`, `exp_avg`, `exp_avg_sq` per parameter), same dense update
rule -- every element moves each step by its decaying momentum, touched by a sample or not.  torch's default foreach
implementation walks the 160 MiB state of a head grid in ~20 multi-tensor kernels; this is one pass per tensor.
CUDA fp32 contiguous parameters only; anything else raises (no silent fallback).

`capturable=True` keeps the step count on the device (like torch.optim.Adam(capturable=True)): no host value is baked into the launch, so a whole
training step can be captured in a HIP graph and replayed (sanerf_hq_amd.graph.GraphedStep).

`lazy=True` (per parameter group, opt-in) switches that group to a touched-elements-only update: an element whose
gradient is exactly zero in a step is skipped altogether (moments do not decay, the parameter does not coast on its momentum) --
torch.optim.SparseAdam's semantics with the non-zeros of the dense gradient as the sparse pattern.  Not the reference's
optimiser: meant for the hash tables, of which a 4096-ray batch touches a few percent of the rows.

`multi_tensor=True` (opt-in; the default route is untouched): one `step()` hands every parameter that has a gradient to
sn_adam_step_multi, at most 32 tensors in 8 groups per call -- one launch for the 13 tensors of the RGB step instead of 13 (26 with
`capturable=True`, whose `step += 1` is a kernel per tensor).  Same arithmetic, bit for bit.  With `capturable=True` the device step
counts are views into one buffer of the optimiser and the kernel advances them itself; the `state_dict` layout stays torch's own, and
a state loaded from elsewhere is packed into that buffer on the next step.

`DeviceLRScale(optimizer, lr_lambda)` is the reference's `LambdaLR` (main.py:298-303) for this route: the factor lives in a device
float that the kernel reads when it RUNS, so a step captured once in a HIP graph follows the schedule.

`ParamEMA(parameters, decay)` is the reference's `torch_ema.ExponentialMovingAverage` (main.py:302 `ema_decay=0.95`; `ema.update()` after
every optimiser step, nerf/trainer.py:1231-1232): the average of every tracked tensor in ONE launch (sn_ema_update_multi), with torch_ema's
warm-up `min(decay, (1 + n) / (10 + n))` formed in the kernel from a count that lives on the device -- so `ema.update()` after
`opt.step()` belongs to the captured step and follows the warm-up under replay.
"""
from __future__ import annotations

import torch

from . import _lib


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False, lazy=False,
                 capturable=False, multi_tensor=False):
        if amsgrad:
            raise ValueError("sanerf_hq_amd.optim.Adam: amsgrad is not implemented (the reference does not use it)")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or weight_decay < 0.0:
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=maximize, lazy=bool(lazy),
                                      capturable=bool(capturable)))
        self.multi_tensor = bool(multi_tensor)       # (an attribute, not a group key: the state_dict is the same on both routes)
        self._lr_scale = None                        # DeviceLRScale: one device float, the factor on every group's initial_lr
        self._counts, self._used, self._slot, self._ticket, self._recs = None, 0, {}, None, None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.lib()
        if self.multi_tensor:
            self._step_multi(lib)
            return loss
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse or not p.is_cuda or p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("sanerf_hq_amd.optim.Adam handles dense contiguous fp32 CUDA parameters only")
                if not g.is_contiguous():
                    g = g.contiguous()
                st = self.state[p]
                cap = bool(group.get("capturable", False))
                if len(st) == 0:
                    # host counter, as torch's non-capturable Adam keeps it; capturable: a device float that the kernel reads when it RUNS
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if cap else torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1                                                   # (capturable: a one-element device kernel, captured with the rest)
                lr = group["lr"]
                _lib.check(lib.sn_adam_step(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(),
                                            float(lr), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                                            0 if cap else int(st["step"].item()), st["step"].data_ptr() if cap else None,
                                            int(bool(group["maximize"])), _lib.ADAM_LAZY if group.get("lazy", False) else 0, _lib.stream()), "sn_adam_step")
                # the kernel wrote through the raw pointer: tell autograd / version-keyed caches (RenderPlan.check_range's fp16
                # range guard, memoised host copies) that the tensor changed, as an in-place torch op would have
                torch.autograd.graph.increment_version(p)
        return loss

    def _count_slot(self, p):
        """A device step count of the capturable multi-tensor route: a 0-dim view into one buffer, so that the kernel's last workgroup
        advances all of them (views stay valid: a full buffer is followed by a new one, never reallocated)."""
        if self._counts is None or self._used == self._counts.numel():
            self._counts = torch.zeros(max(64, sum(len(g["params"]) for g in self.param_groups)), dtype=torch.float32, device=p.device)
            self._used = 0
        slot = self._counts[self._used]
        self._used += 1
        self._slot[p] = slot
        return slot

    def _step_multi(self, lib):
        T, G = _lib.ADAM_MULTI_MAX_TENSORS, _lib.ADAM_MULTI_MAX_GROUPS
        work, device = [], None
        for group in self.param_groups:                                           # the checks of the per-tensor route, before anything is written
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse or not p.is_cuda or p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("sanerf_hq_amd.optim.Adam handles dense contiguous fp32 CUDA parameters only")
                if device is None:
                    device = p.device
                elif p.device != device:
                    raise RuntimeError("sanerf_hq_amd.optim.Adam(multi_tensor=True): all parameters must be on one device")
                work.append((group, p, g if g.is_contiguous() else g.contiguous()))
        if not work:
            return
        if self._recs is None:
            self._recs = ((_lib.AdamTensor * T)(), (_lib.AdamGroup * G)())
        trec, grec = self._recs
        any_cap = any(bool(group.get("capturable", False)) for group, _, _ in work)
        if any_cap and self._ticket is None:
            self._ticket = torch.zeros(1, dtype=torch.int32, device=device)           # zero before first use; every launch leaves it zero
        scale = self._lr_scale.data_ptr() if self._lr_scale is not None else None
        ticket = self._ticket.data_ptr() if any_cap else None
        stream = _lib.stream()
        nt = ng = 0
        current, gi = None, -1
        for group, p, g in work:
            cap = bool(group.get("capturable", False))
            st = self.state[p]
            if len(st) == 0:
                st["step"] = self._count_slot(p) if cap else torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if cap:
                if st["step"] is not self._slot.get(p):                           # a loaded state_dict (or the other route's state): pack the count
                    loaded = st["step"]
                    st["step"] = self._count_slot(p)
                    st["step"].copy_(loaded)
            else:
                st["step"] += 1
            if nt == T or ((group is not current or gi < 0) and ng == G):
                _lib.check(lib.sn_adam_step_multi(trec, nt, grec, ng, scale, ticket, stream), "sn_adam_step_multi")
                nt = ng = 0
                gi = -1
            if group is not current or gi < 0:
                current, gi = group, ng
                r = grec[ng]
                # (with a DeviceLRScale attached group["lr"] is already initial_lr x factor, for logging: the kernel applies the factor itself)
                r.lr = float(group["initial_lr"] if self._lr_scale is not None else group["lr"])
                r.beta1, r.beta2 = float(group["betas"][0]), float(group["betas"][1])
                r.eps, r.weight_decay = float(group["eps"]), float(group["weight_decay"])
                r.maximize, r.flags = int(bool(group["maximize"])), _lib.ADAM_LAZY if group.get("lazy", False) else 0
                ng += 1
            r = trec[nt]
            r.param, r.grad, r.exp_avg, r.exp_avg_sq, r.n = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
            r.step_device, r.step, r.group = (st["step"].data_ptr(), 0, gi) if cap else (None, int(st["step"].item()), gi)
            nt += 1
        _lib.check(lib.sn_adam_step_multi(trec, nt, grec, ng, scale, ticket, stream), "sn_adam_step_multi")
        for _, p, _ in work:
            torch.autograd.graph.increment_version(p)                             # as the per-tensor route: the kernel wrote through raw pointers


class ParamEMA:
    """`torch_ema.ExponentialMovingAverage(parameters, decay, use_num_updates=True)` as the reference's trainer uses it, on the device.

    It tracks exactly the tensors it is given, in order (the reference hands it `model.parameters()`); the shadows are clones.  `update()`
    is torch_ema's statement per element, bit for bit --

        n += 1;  d = min(decay, (1 + n) / (10 + n));  omd = 1.0 - d          # Python doubles (a warm-up: 170 updates at 0.95)
        tmp = s - p;  tmp.mul_(omd);  s.sub_(tmp)                            # fp32 tensors

    -- as ceil(T / 32) calls of sn_ema_update_multi on torch's current stream, one launch each, next to torch_ema's three launches per
    tensor.  `n` is ONE device int64 that the kernel reads when it RUNS and that the last call advances: no host value enters the launch and
    the host reads nothing, so `update()` can be captured in a HIP graph (graph.GraphedStep) after `opt.step()`.  `num_updates` reads the
    count (a host read; None with `use_num_updates=False`, where the decay is constant).

    `store()`, `copy_to()` and `restore()` -- evaluation and checkpoints under the averaged weights, once per epoch -- are `Tensor.copy_`.
    After every write to the parameters (`copy_to`, `restore`) each parameter's version counter is bumped, as `Adam` does, and `on_write()`
    is called once if it was given: pass `model.invalidate_render_plan`, or a model with `render_tables_static = True` goes on rendering
    from half-precision tables converted before the write.

    `state_dict()` has torch_ema's layout, so that checkpoints interchange with the reference's (nerf/trainer.py:1700-1701, 1806-1808):
        {"decay": float, "num_updates": int or None, "shadow_params": [Tensor, ...], "collected_params": None or [Tensor, ...]}
    `load_state_dict()` copies into the existing shadows and the device count.

    Dense contiguous fp32 CUDA tensors only; anything else raises RuntimeError before an element is written (no CPU fallback)."""

    def __init__(self, parameters, decay, use_num_updates=True, on_write=None):
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.decay = decay
        self.on_write = on_write
        self._params = self._checked(list(parameters))
        self.shadow_params = [p.detach().clone() for p in self._params]
        self.collected_params = None
        device = self._params[0].device if self._params else torch.device("cuda")
        self._count = torch.zeros((), dtype=torch.int64, device=device)
        self._ticket = torch.zeros(1, dtype=torch.int32, device=device)           # zero before first use; every launch leaves it zero
        self._use_count = bool(use_num_updates)
        self._recs = None

    @staticmethod
    def _checked(params, like=None):
        """The tensors an entry point may touch, or RuntimeError: nothing has been written when this raises."""
        if like is not None and len(params) != len(like):
            raise ValueError("Number of parameters passed as argument is different from number of shadow parameters maintained by this EMA.")
        for i, p in enumerate(params):
            if not torch.is_tensor(p) or p.is_sparse or not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("sanerf_hq_amd.optim.ParamEMA handles dense contiguous fp32 CUDA parameters only")
            if p.device != params[0].device:
                raise RuntimeError("sanerf_hq_amd.optim.ParamEMA: all parameters must be on one device")
            if like is not None and (p.shape != like[i].shape or p.device != like[i].device):
                raise RuntimeError(f"sanerf_hq_amd.optim.ParamEMA: parameter {i} has shape {tuple(p.shape)} on {p.device}, its shadow {tuple(like[i].shape)} on {like[i].device}")
        return params

    def _parameters(self, parameters):
        return self._params if parameters is None else self._checked(list(parameters), self.shadow_params)

    @property
    def num_updates(self):
        return int(self._count.item()) if self._use_count else None

    @torch.no_grad()
    def update(self, parameters=None):
        params = self._parameters(parameters)
        lib = _lib.lib()
        T = _lib.EMA_MULTI_MAX_TENSORS
        if self._recs is None:
            self._recs = (_lib.EmaTensor * T)()
        recs = self._recs
        count = self._count.data_ptr() if self._use_count else None
        ticket, stream = self._ticket.data_ptr(), _lib.stream()
        for head in range(0, max(len(params), 1), T):                            # (nothing tracked: the count still advances)
            part = range(head, min(head + T, len(params)))
            for r, i in zip(recs, part):
                r.shadow, r.param, r.n = self.shadow_params[i].data_ptr(), params[i].data_ptr(), params[i].numel()
            last = part.stop == len(params)                                       # every call reads count + 1; the last one stores it
            _lib.check(lib.sn_ema_update_multi(recs, len(part), self.decay, count, ticket,
                                               _lib.EMA_ADVANCE if last and self._use_count else 0, stream), "sn_ema_update_multi")

    def _wrote(self, params):
        for p in params:
            torch.autograd.graph.increment_version(p)                             # as Adam: version-keyed caches see the write
        if self.on_write is not None:
            self.on_write()

    @torch.no_grad()
    def copy_to(self, parameters=None):
        """The averaged values into the parameters."""
        params = self._parameters(parameters)
        for s, p in zip(self.shadow_params, params):
            p.data.copy_(s)
        self._wrote(params)

    @torch.no_grad()
    def store(self, parameters=None):
        """Keep a copy of the parameters for `restore()`."""
        self.collected_params = [p.detach().clone() for p in self._parameters(parameters)]

    @torch.no_grad()
    def restore(self, parameters=None):
        """The parameters as `store()` kept them."""
        if self.collected_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        params = self._parameters(parameters)
        for c, p in zip(self.collected_params, params):
            p.data.copy_(c)
        self._wrote(params)

    def state_dict(self):
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": self.shadow_params, "collected_params": self.collected_params}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        decay, n = float(state_dict["decay"]), state_dict["num_updates"]
        if not 0.0 <= decay <= 1.0:
            raise ValueError("Decay must be between 0 and 1")
        if n is not None and (not isinstance(n, int) or n < 0):
            raise ValueError("Invalid num_updates")
        shadows, collected = state_dict["shadow_params"], state_dict["collected_params"]
        for name, ts in (("shadow_params", shadows), ("collected_params", collected)):
            if name == "collected_params" and ts is None:
                continue
            if not isinstance(ts, (list, tuple)) or not all(torch.is_tensor(t) for t in ts):
                raise ValueError(f"{name} must all be Tensors")
            if len(ts) != len(self.shadow_params) or any(t.shape != s.shape for t, s in zip(ts, self.shadow_params)):
                raise ValueError(f"{name} does not match the tensors this EMA tracks")
        self.decay = decay
        self._use_count = n is not None
        self._count.fill_(n if n is not None else 0)
        for s, t in zip(self.shadow_params, shadows):
            s.copy_(t)
        self.collected_params = None if collected is None else [t.detach().to(device=s.device, dtype=s.dtype, copy=True) for t, s in zip(collected, self.shadow_params)]


class DeviceLRScale:
    """`torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda)` for `Adam(multi_tensor=True)`, with the factor on the device.

    `step()` evaluates `lr_lambda(it)` on the host, writes it into the optimiser's one-element device tensor (from pinned memory,
    without blocking) and sets `group["lr"] = initial_lr * factor`, which is what LambdaLR would show.  The kernel is handed
    `initial_lr` and reads the factor when it runs -- eagerly, or at every replay of a `GraphedStep` that captured `optimizer.step()`.
    As with LambdaLR, constructing it performs the step for iteration 0."""
    _RING = 8

    def __init__(self, optimizer, lr_lambda):
        if not isinstance(optimizer, Adam) or not optimizer.multi_tensor:
            raise TypeError("DeviceLRScale needs a sanerf_hq_amd.optim.Adam(multi_tensor=True): the per-tensor route takes its rate from the host")
        if optimizer._lr_scale is not None:
            raise RuntimeError("this optimiser already has a DeviceLRScale attached")
        self.optimizer, self.lr_lambda = optimizer, lr_lambda
        for group in optimizer.param_groups:
            group.setdefault("initial_lr", group["lr"])
        self.base_lrs = [group["initial_lr"] for group in optimizer.param_groups]
        device = optimizer.param_groups[0]["params"][0].device
        self._factor_dev = torch.ones(1, dtype=torch.float32, device=device)
        # the copy reads the pinned word when the STREAM reaches it: a ring of words, each reused only once its copy has run
        self._ring = torch.ones(self._RING, dtype=torch.float32).pin_memory() if device.type == "cuda" else None
        self._events = [torch.cuda.Event() for _ in range(self._RING)] if device.type == "cuda" else None
        self._writes = 0
        optimizer._lr_scale = self._factor_dev
        self.last_epoch = -1
        self.factor = 1.0
        self.step()

    def _apply(self, factor):
        self.factor = float(factor)
        if self._ring is None:
            self._factor_dev.fill_(self.factor)
        else:
            i = self._writes % self._RING
            self._writes += 1
            self._events[i].synchronize()                  # (returns at once unless the host is a whole ring of steps ahead of the device)
            word = self._ring[i:i + 1]
            word.fill_(self.factor)
            self._factor_dev.copy_(word, non_blocking=True)
            self._events[i].record()
        for group, base in zip(self.optimizer.param_groups, self.base_lrs):
            group["lr"] = base * self.factor

    def step(self):
        self.last_epoch += 1
        self._apply(self.lr_lambda(self.last_epoch))

    def get_last_lr(self):
        return [group["lr"] for group in self.optimizer.param_groups]

    def state_dict(self):
        return {"last_epoch": self.last_epoch, "base_lrs": list(self.base_lrs), "factor": self.factor}

    def load_state_dict(self, state):
        self.last_epoch, self.base_lrs = int(state["last_epoch"]), list(state["base_lrs"])
        for group, base in zip(self.optimizer.param_groups, self.base_lrs):
            group["initial_lr"] = base
        self._apply(state["factor"])
