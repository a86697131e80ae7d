"""An exponential moving average (EMA) of the parameters, kept beside the optimizer state: the weights to synthesise and score with.

The fused optimizers hold every parameter as a view of one flat fp32 buffer (`FlatOptimizer.flat_p`, the engine's gradient layout), so the
average is one more flat buffer of that layout and one update is ONE streaming launch behind the optimizer's (efts_ema_update:
e = fmaf(w, p - e, e), 3 words per element), with its one word w = 1 - decay from the host (efts_ema_hyper; with `warmup` the decay is
min(decay, (1 + n) / (10 + n)) at update n, so a short run is not dominated by the initial weights).  `FlatOptimizer.step()` and
`GraphedStep.__call__` call `update()` right behind their own launches, on the same stream, with the same words: the captured graph of a
step is not touched.

Data parallel: every rank holds identical parameters behind the all-reduce, so every rank updates its own copy of the average from its
own copy of the parameters.  No collective, and the copies stay identical bit for bit (the launch has no atomics).
"""
from __future__ import annotations

import contextlib
import ctypes as C

import torch

from . import lib as L
from . import ops as O
from .optim import FlatOptimizer


class ParamEMA:
    """ema = ParamEMA(optimizer, decay=0.999, warmup=True); attaches itself as `optimizer.ema`, from where the step calls `update()`.

    flat     the averaged parameters: a clone of `optimizer.flat_p` at construction, same layout and offsets
    updates  updates made so far (host int)"""

    def __init__(self, optimizer, decay: float = 0.999, warmup: bool = True):
        if not isinstance(optimizer, FlatOptimizer):
            raise TypeError(f"ParamEMA needs one of the fused optimizers (efficient_tts_amd.optim.FlatOptimizer: Adam, AdamW, RAdam of the "
                            f"registry), whose parameters live in one flat buffer; got {type(optimizer).__name__}")
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError(f"ema decay must lie in (0, 1), got {decay!r}")
        L.require_device()
        self.opt = optimizer
        self.decay, self.warmup = decay, bool(warmup)
        self.flat = optimizer.flat_p.clone()
        self.updates = 0
        self._scratch = None                    # the one buffer `applied()` exchanges through, allocated at its first use
        self._applied = False
        optimizer.ema = self

    # ---------------------------------------------------------------------------------------------- the update
    def word(self) -> float:
        """1 - decay of the update about to be made, as efts_ema_hyper rounds it to fp32"""
        arr = (C.c_float * 1)()
        L.check(L.load().efts_ema_hyper(self.decay, int(self.warmup), int(self.updates), arr), "efts_ema_hyper")
        return float(arr[0])

    @torch.no_grad()
    def update(self) -> None:
        """one efts_ema_update launch on the library's stream; nothing is read back"""
        if self._applied:
            raise RuntimeError("ParamEMA.update() inside applied(): the model holds the averaged weights")
        L.check(L.load().efts_ema_update(self.flat.data_ptr(), self.opt.flat_p.data_ptr(), self.opt.eng.numel, self.word(), O._stream()),
                "efts_ema_update")
        self.updates += 1

    @torch.no_grad()
    def reset(self) -> None:
        """the average starts over from the current parameters"""
        if self._applied:
            raise RuntimeError("ParamEMA.reset() inside applied()")
        self.flat.copy_(self.opt.flat_p)
        self.updates = 0

    # ---------------------------------------------------------------------------------------------- the averaged weights in the model
    def _exchange(self) -> None:
        if self._scratch is None:
            self._scratch = torch.empty_like(self.flat)
        p, e, s = self.opt.flat_p, self.flat, self._scratch
        s.copy_(p); p.copy_(e); e.copy_(s)
        self.opt.model.planes.invalidate()      # parameters changed in place through the flat view

    @contextlib.contextmanager
    def applied(self):
        """`with ema.applied():` the model computes with the averaged weights; behind the block it holds the raw ones again, bit for bit.
        The CONTENTS of `flat_p` and `flat` are exchanged (device copies through one scratch buffer), no parameter is re-pointed: a captured
        training step keeps its pointers and its tag and replays afterwards.  Not re-entrant."""
        if self._applied:
            raise RuntimeError("ParamEMA.applied() is already active: it does not nest")
        with torch.no_grad():
            self._exchange()
        self._applied = True
        try:
            yield self
        finally:
            self._applied = False
            with torch.no_grad():
                self._exchange()

    # ---------------------------------------------------------------------------------------------- state
    def _averaged(self) -> torch.Tensor:
        return self.opt.flat_p if self._applied else self.flat

    def state_dict(self) -> dict:
        """{"decay", "warmup", "updates", "model"}: "model" is the averaged parameters under the model's reference `state_dict` keys
        (weight_g / weight_v averaged as the parameters they are), non-parameter entries copied from the model: it loads wherever a
        checkpoint's "model" entry does"""
        eng, flat = self.opt.eng, self._averaged()
        model = {}
        for key, value in self.opt.model.state_dict().items():
            if key in eng.offsets:
                a, b = eng.offsets[key]
                model[key] = flat[a:b].view(value.shape).clone()
            else:
                model[key] = value.detach().clone()
        return dict(decay=self.decay, warmup=self.warmup, updates=int(self.updates), model=model)

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        """restores the average and the update count (decay and warm-up stay what this object was built with)"""
        if self._applied:
            raise RuntimeError("ParamEMA.load_state_dict() inside applied()")
        eng = self.opt.eng
        own = set(self.opt.model.state_dict())
        want, have = set(eng.offsets), set(sd["model"]) - (own - set(eng.offsets))
        if want != have:
            raise ValueError(f"the averaged parameters do not fit this model: missing {sorted(want - have)}, unexpected {sorted(have - want)}")
        for name, (a, b) in eng.offsets.items():
            value = sd["model"][name]
            if value.numel() != b - a:
                raise ValueError(f"the averaged parameter {name} has {value.numel()} elements, the model's has {b - a}")
            self.flat[a:b].copy_(value.reshape(-1))
        self.updates = int(sd["updates"])
