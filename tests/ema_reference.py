"""The exponential moving average of the parameters, restated: the per-update word in Python floats, the recurrence in numpy float64.
What tests/test_ema_cpu.py holds efts_ema_hyper against and tests/test_ema_gpu.py holds efts_ema_update and ParamEMA against."""
import struct

import numpy as np

EPS = 2.0 ** -23          # per element and update: |device - exact| <= EPS (|p| + |e|), see `bound`


def f32(x: float) -> float:
    """x rounded to fp32 once, as a Python float"""
    return struct.unpack("f", struct.pack("f", x))[0]


def decay_at(decay: float, warmup: bool, updates: int) -> float:
    """the decay of the update made after `updates` updates (0 for the first)"""
    return min(decay, (1 + updates) / (10 + updates)) if warmup else decay


def word(decay: float, warmup: bool, updates: int) -> float:
    """1 - decay of that update, rounded to fp32 once: what efts_ema_hyper returns"""
    return f32(1.0 - decay_at(decay, warmup, updates))


def update(e, p, w: float):
    """one update in float64: e + w (p - e), no rounding that matters at fp32's scale.  w is the fp32 word as a Python float."""
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return e + w * (p - e)


def bound(e, p):
    """what one fp32 update e' = fma(w, fl(p - e), e) may differ by from `update` for w in [0, 1], per element: the subtraction loses at most
    2^-24 |p - e|, scaled by w <= 1, and the fma's one rounding at most 2^-24 |e'| with |e'| <= max(|p|, |e|); together under
    2^-23 (|p| + |e|)"""
    return EPS * (np.abs(np.asarray(p, dtype=np.float64)) + np.abs(np.asarray(e, dtype=np.float64)))


def run(e0, snapshots, decay: float, warmup: bool, updates0: int = 0):
    """the recurrence over `snapshots` (the parameters after every step) from e0, with the words of updates updates0, updates0 + 1, ...
    Returns (the average in float64, the summed per-update bounds).  The recurrence is a contraction -- an error d in e becomes (1 - w) d --
    so what earlier updates lost does not grow, and the device may differ from this by the sum of the per-update bounds at the most."""
    e = np.asarray(e0, dtype=np.float64).copy()
    total = np.zeros_like(e)
    for k, p in enumerate(snapshots):
        total += bound(e, p)
        e = update(e, p, word(decay, warmup, updates0 + k))
    return e, total
