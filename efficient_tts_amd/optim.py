"""Optimizer and schedule of the reference recipe, fused for MI355X.

* `EftsAdam` -- torch.optim.Adam(lr, betas, eps, weight_decay (coupled L2), amsgrad)
  (egs/lj/conf/efficient_tts_cnn_phnseq_noDropout.v1.yaml:34-40) as ONE HBM-bound kernel over flat
  fp32 buffers, with `clip_grad_norm_` (trainer.py:154-157) folded in: the global-norm reduction
  stays on the device, no host sync per step.  Parameters are re-homed as views of one flat buffer
  in the engine's gradient layout (so data-parallel buckets are contiguous).
* `EftsAdamW`, `EftsRAdam` -- torch.optim.AdamW and the reference's own RAdam (nntts/optimizers/radam.py), the same
  way (`FlatOptimizer`): what `optimizer_type` may name besides Adam.
* `WarmupLR` -- nntts/schedulers/warmup_lr.py:9-51: lr * w^0.5 * min(s^-0.5, s * w^-1.5).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.optim.lr_scheduler import _LRScheduler

from . import lib as L
from . import ops as O
from .autograd import engine_of
from .model import require_trainable


class _OptimStepKernel:
    """efts_optim_step: every member of the family but the recipe's amsgrad Adam.  Four per-step words (efts_optim_hyper), words 4-7 of
    GraphedStep's eight device words (word 3 is the Dropout step word)."""
    word0 = 4

    @staticmethod
    def words(opt, step):
        grp = opt.param_groups[0]
        arr = (C.c_float * 4)()
        L.check(L.load().efts_optim_hyper(opt.ALGO, float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1]), float(grp["weight_decay"]),
                                          int(step), arr), "efts_optim_hyper")
        return list((C.c_uint32 * 4).from_buffer(arr))

    @staticmethod
    def launch(opt, sumsq, grad_scale, hyper_ptr, st):
        eng, grp = opt.eng, opt.param_groups[0]
        a = L.OptimArgs()
        a.p, a.g, a.m, a.v, a.n = opt.flat_p.data_ptr(), eng.flat.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr(), eng.numel
        a.vmax = opt.vmax.data_ptr() if opt.amsgrad else None
        a.sumsq, a.max_norm, a.gscale = sumsq, opt.grad_norm, float(grad_scale)
        a.algo, a.amsgrad = opt.ALGO, int(opt.amsgrad)
        a.lr, a.beta1, a.beta2 = float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1])
        a.eps, a.weight_decay = float(grp["eps"]), float(grp["weight_decay"])
        a.step, a.hyper = opt.t, hyper_ptr
        L.check(L.load().efts_optim_step(a, st), "efts_optim_step")


class _AmsgradAdamKernel:
    """efts_adam_amsgrad / efts_adam_amsgrad_dev: the kernel of the shipped recipe (Adam, coupled L2, amsgrad), kept bit for bit.  Three
    per-step words {lr, 1 - beta1^step, sqrt(1 - beta2^step)} (efts_adam_hyper), words 0-2 of GraphedStep's eight."""
    word0 = 0

    @staticmethod
    def words(opt, step):
        grp = opt.param_groups[0]
        arr = (C.c_float * 3)()
        L.check(L.load().efts_adam_hyper(float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1]), int(step), arr), "efts_adam_hyper")
        return list((C.c_uint32 * 3).from_buffer(arr))

    @staticmethod
    def launch(opt, sumsq, grad_scale, hyper_ptr, st):
        eng, grp, lib = opt.eng, opt.param_groups[0], L.load()
        bufs = (opt.flat_p.data_ptr(), eng.flat.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr(), opt.vmax.data_ptr(), eng.numel, sumsq,
                opt.grad_norm, float(grad_scale))
        rest = (float(grp["betas"][0]), float(grp["betas"][1]), float(grp["eps"]), float(grp["weight_decay"]))
        if hyper_ptr is None:
            L.check(lib.efts_adam_amsgrad(*bufs, float(grp["lr"]), *rest, opt.t, st), "efts_adam_amsgrad")
        else:
            L.check(lib.efts_adam_amsgrad_dev(*bufs, hyper_ptr, *rest, st), "efts_adam_amsgrad_dev")


class FlatOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: the parameters re-homed as views of ONE flat buffer in the engine's gradient layout, the moments
    as flat buffers beside it, the on-device global norm, and a step that is `launch()` -- clip + update in one kernel over the flat
    buffers -- plus host bookkeeping.  A subclass names its algorithm (`ALGO`, EFTS_OPTIM_*) and its state-dict layout; `kernel` is the
    launch behind it (efts_optim_step unless a subclass picks another)."""
    ALGO = None

    def __init__(self, model, defaults, amsgrad, grad_norm, kernel=_OptimStepKernel):
        name = type(self).__name__
        require_trainable(model, name)
        self.model = model
        self.eng = engine_of(model)
        eng = self.eng
        eng.bound.add(name)
        self.grad_norm = float(grad_norm)
        self.amsgrad = bool(amsgrad)
        self._kernel = kernel
        self.hyper_word0 = kernel.word0         # where GraphedStep keeps `hyper_words` in its eight device words
        dev = eng.dev
        # re-home parameters into one flat buffer (engine layout)
        self.flat_p = torch.empty_like(eng.flat)
        with torch.no_grad():
            for n, p in eng.layout:
                a, b = eng.offsets[n]
                self.flat_p[a:b].copy_(p.detach().reshape(-1))
                p.data = self.flat_p[a:b].view_as(p)
        self.m = torch.zeros_like(eng.flat)
        self.v = torch.zeros_like(eng.flat)
        self.vmax = torch.zeros_like(eng.flat) if self.amsgrad else None
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.sumsq_ws = torch.zeros(L.load().efts_sumsq_workspace_bytes() // 4, dtype=torch.float32, device=dev)
        self.t = 0
        self.ema = None                         # an attached ema.ParamEMA: updated behind every step's launch
        super().__init__([p for _, p in eng.layout], defaults)

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        """clip (global norm of grad_scale * flat grads) + update, all on the device."""
        self.t += 1
        self.launch(grad_scale)
        if self.ema is not None:
            self.ema.update()
        self.model.planes.invalidate()          # parameters changed in place through the flat view

    def hyper_words(self, step: int):
        """the per-step words of the kernel as it derives them from its by-value arguments, as 32-bit words"""
        return self._kernel.words(self, step)

    def _sumsq_ptr(self, st):
        """the launches of the global gradient norm; the device address of sum(g^2), or None without a clip"""
        if self.grad_norm <= 0:
            return None
        eng = self.eng
        self.sumsq.zero_()
        L.check(L.load().efts_sumsq(eng.flat.data_ptr(), eng.numel, self.sumsq.data_ptr(), self.sumsq_ws.data_ptr(), st), "efts_sumsq")
        return self.sumsq.data_ptr()

    @torch.no_grad()
    def launch(self, grad_scale: float = 1.0, hyper_ptr=None):
        """the launches of step() for step number `self.t`, nothing else.  hyper_ptr: device floats, the words of `hyper_words`, read by the
        kernel instead of the by-value scalars (a step captured as a hipGraph: step_graph.GraphedStep)."""
        st = O._stream()
        self._kernel.launch(self, self._sumsq_ptr(st), grad_scale, hyper_ptr, st)

    def zero_grad(self, set_to_none: bool = True):
        for _, p in self.eng.layout:
            p.grad = None

    # ---- state: torch's layout, numbered in model.parameters() order (nntts/bin/train.py:196-205), so that `--resume` works across this
    # implementation and the optimizer it replaces (nntts/trainers/efficient_tts_trainer.py:90-103 saves optimizer.state_dict() as is)
    def _step_entry(self):
        return torch.tensor(float(self.t))

    def _group_extras(self) -> dict:
        return {}

    def state_dict(self):
        eng, state = self.eng, {}
        names = [n for n, _ in self.model.named_parameters()]
        for i, n in enumerate(names):
            a, b = eng.offsets[n]
            shape = dict(eng.layout)[n].shape
            state[i] = dict(step=self._step_entry(), exp_avg=self.m[a:b].view(shape).clone(), exp_avg_sq=self.v[a:b].view(shape).clone())
            if self.amsgrad:
                state[i]["max_exp_avg_sq"] = self.vmax[a:b].view(shape).clone()
        groups = []
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != "params"}
            d.update(self._group_extras())
            d.update(params=list(range(len(names))))
            groups.append(d)
        return dict(state=state, param_groups=groups)

    def load_state_dict(self, sd):
        eng = self.eng
        if "state" in sd:                                        # torch layout (ours or the reference's)
            names = [n for n, _ in self.model.named_parameters()]
            if len(sd["state"]) not in (0, len(names)):
                raise ValueError(f"optimizer state holds {len(sd['state'])} parameters, the model has {len(names)}")
            steps = set()
            for i, n in enumerate(names):
                st = sd["state"].get(i)
                if st is None:
                    continue
                a, b = eng.offsets[n]
                self.m[a:b].copy_(st["exp_avg"].reshape(-1))
                self.v[a:b].copy_(st["exp_avg_sq"].reshape(-1))
                if self.amsgrad:
                    self.vmax[a:b].copy_(st.get("max_exp_avg_sq", st["exp_avg_sq"]).reshape(-1))
                steps.add(int(float(st["step"])))
            if len(steps) > 1:
                raise ValueError(f"per-parameter step counts differ ({sorted(steps)}): the fused kernel keeps one")
            self.t = steps.pop() if steps else 0
        else:                                                    # round-1 flat layout
            self.t = int(sd["t"])
            self.m.copy_(sd["m"]); self.v.copy_(sd["v"])
            if self.amsgrad:
                self.vmax.copy_(sd["vmax"])
        for g, s_ in zip(self.param_groups, sd["param_groups"]):
            g.update({k: v for k, v in s_.items() if k in ("lr", "betas", "eps", "weight_decay", "initial_lr")})


class EftsAdam(FlatOptimizer):
    """torch.optim.Adam (coupled L2).  amsgrad=True (the reference YAML) keeps its own kernel, efts_adam_amsgrad, bit for bit."""
    ALGO = L.OPTIM_ADAM

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.99), eps=1e-9, weight_decay=1e-5, amsgrad=True, grad_norm=1.0):
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), amsgrad, grad_norm,
                         kernel=_AmsgradAdamKernel if amsgrad else _OptimStepKernel)

    def _group_extras(self):
        return dict(amsgrad=self.amsgrad, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)


class EftsAdamW(FlatOptimizer):
    """torch.optim.AdamW (decoupled decay: p *= 1 - lr * weight_decay in front of the Adam update)"""
    ALGO = L.OPTIM_ADAMW

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, grad_norm=1.0):
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), amsgrad, grad_norm)

    def _group_extras(self):
        return dict(amsgrad=self.amsgrad, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                    decoupled_weight_decay=True)


class EftsRAdam(FlatOptimizer):
    """The reference's RAdam (nntts/optimizers/radam.py), not torch.optim.RAdam: rectified from N_sma >= 5, eps outside the bias
    correction, decoupled decay.  State as that file keeps it: {step: int, exp_avg, exp_avg_sq} per parameter."""
    ALGO = L.OPTIM_RADAM

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, grad_norm=1.0):
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), False, grad_norm)

    def _step_entry(self):
        return int(self.t)


class WarmupLR(_LRScheduler):
    """lr = base_lr * warmup^0.5 * min(step^-0.5, step * warmup^-1.5), step = last_epoch + 1
    (nntts/schedulers/warmup_lr.py:44-51)."""

    def __init__(self, optimizer, warmup_steps=25000, last_epoch=-1):
        self.warmup_steps = warmup_steps
        super().__init__(optimizer, last_epoch)

    def __repr__(self):
        return f"{self.__class__.__name__}(warmup_steps={self.warmup_steps})"

    def get_lr(self):
        s = self.last_epoch + 1
        return [lr * self.warmup_steps ** 0.5 * min(s ** -0.5, s * self.warmup_steps ** -1.5) for lr in self.base_lrs]
