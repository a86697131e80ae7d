"""The train-mode Dropout masks of one pass: which (p, seed) its launches carry.  Pure arithmetic, no device work.  One mask family
per (model seed, data-parallel rank, step): the training step (train._Step.drop) and the gradient-free train()-mode forward
(model._Pass.drop) read the same `DropoutPlan` for the same step, and the backward regenerates the masks from the same seeds."""
from __future__ import annotations

import dataclasses
from typing import Optional

M32 = 0xFFFFFFFF
# index k of the Dropout behind conv / prenet launch k: layer i of a stack is <stack> + i (a stack that is none of the three: other + i)
LAUNCH = {"te": 10, "me": 20, "dec": 30, "prenet": 40, "other": 50}


def rank_base(seed: int, rank: int) -> int:
    """the base seed of one process's mask family (the reference's ranks have their own torch RNG streams)"""
    return (int(seed) + 0x9E3779B1 * rank) & M32


def dist_rank() -> int:
    """the data-parallel rank of this process (0 without an initialised torch.distributed)"""
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


@dataclasses.dataclass(frozen=True)
class DropoutPlan:
    """conv_p / dur_p: the rates of the ResConv1d + prenet Dropouts and of the duration predictor's (0: off); base: rank_base(); calls: the
    step drawn; step_word_ptr: a step that is being captured as a hipGraph (step_graph.GraphedStep) takes the step's share of the duration seeds
    from this device word (= step_word(calls), refreshed in front of every replay); its by-value seeds stay constant.  (Conv seeds: by value only)"""
    conv_p: float
    dur_p: float
    base: int
    calls: int
    step_word_ptr: Optional[int] = None

    @property
    def conv_active(self) -> bool:
        return self.conv_p > 0.0

    def conv(self, k: int):
        """(p, seed) of the Dropout behind the activation of conv / prenet launch k (efts_modules.py:38-47, efficient_tts.py:76-80)"""
        if not self.conv_active:
            return 0.0, 0
        return self.conv_p, (self.base * 2654435761 + self.calls * 1000003 + k * 7919 + 12345) & M32

    def dur(self, i: int):
        """(p, seed, seed_add_ptr) of the Dropout behind LayerNorm i of the duration predictor (duration_predictor.py:61); the kernels add the word at the pointer"""
        if self is NONE:
            return 0.0, 0, None
        step = 0 if self.step_word_ptr is not None else self.step_word(self.calls)
        return self.dur_p, (self.base + step + (min(i, 1) if i < 2 else 1 + i)) & M32, self.step_word_ptr

    @staticmethod
    def step_word(calls: int) -> int:
        return 2 * calls


NONE = DropoutPlan(0.0, 0.0, 0, 0)          # eval, inference and align(): no Dropout, seed 0 in every launch
