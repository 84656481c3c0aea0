"""The optimizer state every trainer of the package shares: ONE flat fp32 parameter buffer with its gradient, AdamW moments, optional EMA
shadow and optional gradient accumulator, addressed by a ``layout`` of ``name -> (offset, shape)``.  The step is two kernels over the flat
buffers (``dfot_sumsq`` for the global gradient norm, ``dfot_adamw_step`` for clip + AdamW + EMA); data parallelism is one all-reduce of the
flat gradient.  ``FlatAdamW`` is the state, ``FlatAdamWOwner`` what a trainer that holds one (``self.opt``) exposes of it.

Mirrors ``BasePytorchAlgo.configure_optimizers`` (AdamW + Lightning's gradient_clip_val), ``accumulate_grad_batches`` /
``accelerator.accumulate`` (simple_video_generation.py:260) and ``EMAModel`` (algorithms/common/ema.py: shadow = decay * shadow +
(1 - decay) * param after every optimizer step; ema.safetensors, simple_video_generation.py:653-657)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import capi, parallel

Layout = Dict[str, Tuple[int, Tuple[int, ...]]]


class FlatAdamW:
    def __init__(self, layout: Layout, numel: int, device="cuda"):
        """device: anything but the default only serves host tests of the torch-only parts (views, accumulation, state dicts)"""
        self.layout, self.numel = layout, int(numel)
        self.params = torch.zeros(self.numel, device=device, dtype=torch.float32)
        self.grads = torch.zeros_like(self.params)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self._sumsq = torch.zeros(1, device=device, dtype=torch.float32)
        self.step_count = 0
        self.ema: Optional[torch.Tensor] = None  # EMAModel shadow weights (flat), updated inside the optimizer kernel
        self.ema_decay = 0.0
        self._acc: Optional[torch.Tensor] = None
        self._acc_n = 0
        self._acc_reduced = True  # every accumulated micro-batch gradient was already averaged over the ranks

    def view(self, name: str, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
        off, shape = self.layout[name]
        return (self.params if buf is None else buf)[off: off + int(np.prod(shape))].view(shape)

    # ------------------------------------------------------------------ accumulation and the step
    def accumulate(self, reduced: bool = False) -> None:
        """add `grads` to the running sum; the next step uses the MEAN over the accumulated micro-batches.  reduced: this gradient is
        already the mean over the ranks -- the reference reduces once per optimizer step (the micro-batches run under no_sync), so the
        accumulated mean needs no exchange of its own only if ALL its micro-batches were reduced"""
        if self._acc is None:
            self._acc = torch.zeros_like(self.grads)
        if self._acc_n == 0:
            self._acc_reduced = True
        self._acc_reduced = self._acc_reduced and bool(reduced)
        self._acc.add_(self.grads)
        self._acc_n += 1

    def take_accumulated(self) -> bool:
        """grads <- the mean of the accumulated gradients, if there are any (returns whether)"""
        if not self._acc_n:
            return False
        self.grads.copy_(self._acc).mul_(1.0 / self._acc_n)
        self._acc.zero_()
        self._acc_n = 0
        return True

    def _grad_sumsq(self) -> torch.Tensor:
        capi.check(capi.lib.dfot_sumsq(capi.ptr(self.grads), self.numel, capi.ptr(self._sumsq), capi.stream_ptr()))
        return self._sumsq

    def grad_norm(self) -> float:
        return float(self._grad_sumsq().sqrt().item())

    def step(self, lr: float, betas, eps: float, weight_decay: float, max_grad_norm: Optional[float], world_size: int = 1,
             grads_reduced: bool = False) -> None:
        """[mean of the accumulated gradients] -> [all-reduce + average the flat gradient] -> global-norm clip -> AdamW, the EMA shadow
        updated by the same kernel pass that writes the new parameters"""
        if self.take_accumulated():
            grads_reduced = self._acc_reduced  # local micro-batch gradients: ONE exchange of the accumulated mean, here
        if world_size > 1 and not grads_reduced:
            parallel.allreduce_mean_(self.grads)
        self.step_count += 1
        sumsq = self._grad_sumsq() if max_grad_norm is not None else None
        capi.check(capi.lib.dfot_adamw_step(capi.ptr(self.params), capi.ptr(self.grads), capi.ptr(self.exp_avg), capi.ptr(self.exp_avg_sq),
                                            self.numel, lr, betas[0], betas[1], eps, weight_decay, self.step_count, capi.ptr(sumsq),
                                            float(max_grad_norm or 0.0), capi.ptr(self.ema), float(self.ema_decay), capi.stream_ptr()))

    # ------------------------------------------------------------------ EMA and optimizer state (checkpoint / resume)
    def enable_ema(self, decay: float) -> None:
        """experiment.ema (algorithms/common/ema.py): shadow weights start as a copy of the parameters"""
        self.ema, self.ema_decay = self.params.clone(), float(decay)

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """what the reference writes to ema.safetensors: the shadow of every trainable parameter"""
        if self.ema is None:
            raise RuntimeError("EMA is not enabled")
        return {k: self.view(k, self.ema).detach().clone() for k in self.layout}

    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        if self.ema is None:
            raise RuntimeError("EMA is not enabled")
        if set(sd.keys()) != set(self.layout.keys()):
            raise ValueError("The provided state_dict does not match the structure of the EMA model.")
        for k, t in sd.items():
            self.view(k, self.ema).copy_(t.to(device=self.ema.device, dtype=torch.float32))

    def optimizer_state_dict(self, hyper: Dict) -> Dict:
        """torch.optim.AdamW.state_dict() layout (parameter index = position in the reference's parameter order); hyper: lr, betas, eps,
        weight_decay of the one parameter group"""
        state = {i: {"step": torch.tensor(float(self.step_count)), "exp_avg": self.view(k, self.exp_avg).clone(),
                     "exp_avg_sq": self.view(k, self.exp_avg_sq).clone()} for i, k in enumerate(self.layout)} if self.step_count else {}
        group = dict(lr=hyper["lr"], betas=hyper["betas"], eps=hyper["eps"], weight_decay=hyper["weight_decay"], amsgrad=False,
                     params=list(range(len(self.layout))))
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd: Dict) -> Optional[Dict]:
        """-> the hyper-parameters of the first parameter group (None: the dict has no group)"""
        names = list(self.layout)
        steps = set()
        for i, st in sd.get("state", {}).items():
            k = names[int(i)]
            self.view(k, self.exp_avg).copy_(st["exp_avg"].to(self.exp_avg.device))
            self.view(k, self.exp_avg_sq).copy_(st["exp_avg_sq"].to(self.exp_avg_sq.device))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ: the flat optimizer keeps one")
        self.step_count = steps.pop() if steps else 0
        if not sd.get("param_groups"):
            return None
        g0 = sd["param_groups"][0]
        return dict(lr=g0["lr"], betas=tuple(g0["betas"]), eps=g0["eps"], weight_decay=g0["weight_decay"])


def alias(name: str) -> property:
    """a trainer attribute that reads and writes `self.opt.<name>`: the same storage, no copy"""
    return property(lambda self: getattr(self.opt, name), lambda self, value: setattr(self.opt, name, value))


class FlatAdamWOwner:
    """A trainer that holds one FlatAdamW as ``self.opt``: the state's names and the methods that are the same for every trainer.  The
    trainer supplies ``_hyper`` (dict of lr / betas / eps / weight_decay, readable and writable: the parameter group of the state dict) and
    its own ``optimizer_step``: how the hyper-parameters arrive and what follows a step differ between the families."""

    exp_avg, exp_avg_sq = alias("exp_avg"), alias("exp_avg_sq")
    ema, ema_decay = alias("ema"), alias("ema_decay")
    _acc, _acc_n = alias("_acc"), alias("_acc_n")
    step_count = alias("step_count")
    _grads_reduced = False  # the gradient of the last backward is already the mean over the ranks (set by a trainer that can overlap the exchange)

    def view(self, name: str, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.opt.view(name, buf)

    def accumulate(self) -> None:
        """accumulate_grad_batches: add the gradients of the last backward to the running sum used by the next optimizer_step"""
        self.opt.accumulate(self._grads_reduced)

    def enable_ema(self, decay: float) -> None:
        self.opt.enable_ema(decay)

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        return self.opt.ema_state_dict()

    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        self.opt.load_ema_state_dict(sd)

    def optimizer_state_dict(self) -> Dict:
        return self.opt.optimizer_state_dict(self._hyper)

    def load_optimizer_state_dict(self, sd: Dict) -> None:
        hyper = self.opt.load_optimizer_state_dict(sd)
        if hyper is not None:
            self._hyper = hyper

    def grad_norm(self) -> float:
        return self.opt.grad_norm()
