"""On-device IIR filtering of a padded batch: a cascade of up to four second-order sections in fp64, and the closed-form designs that the audio
path needs in front of its other steps -- a Butterworth high-pass against DC and rumble, pre-emphasis and its inverse.

With the sections (b0, b1, b2, a1, a2), a0 = 1, run in order on every sample, each in transposed direct form II from zero state:

    y = b0 x + s1;  s1 = b1 x - a1 y + s2;  s2 = b2 x - a2 y              out = fp32(y of the last section), 0 behind an item's length

include/efts_abi.h has the definition to the bit.  The recurrence runs in csrc/efts_iir.hip (`efts_iir` and its `_pcm16` twin) without the
dependent chain over the whole item: a thread runs a segment of 256 samples from zero state, a wave per item carries the exact state across
the segments with the transition matrices built here (`transition_powers`), and a second pass re-runs every segment from its true start
state.  Three launches per call, no atomics, nothing read back by the host.  The filter is causal only (no zero-phase mode), starts from
zero state, has at most 4 sections, writes fp32 and has no backward pass.  No CPU path: the HIP library is required.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np
import torch

from . import audio_args as A
from . import lib as L_
from . import ops as O

SEGMENT = 256            # EFTS_IIR_SEGMENT: samples of one thread
MAX_SECTIONS = 4         # EFTS_IIR_MAX_SECTIONS
SCAN_STEPS = 6           # M^(2^k) for k = 0 .. 5: the scan over the 64 lanes of a wave


# ---------------------------------------------------------------------------------------------- designs
def check_sos(sos) -> np.ndarray:
    """float64 [K, 5] (b0, b1, b2, a1, a2) from [K, 5] or scipy's [K, 6] with a0 == 1; refuses anything but 1 .. 4 finite sections whose
    poles all lie inside the unit circle (|a2| < 1 and |a1| < 1 + a2)."""
    s = np.array(sos, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] not in (5, 6):
        raise ValueError(f"sos must be [K, 5] (b0, b1, b2, a1, a2) or [K, 6] (b0, b1, b2, a0 = 1, a1, a2), got shape {s.shape}")
    if s.shape[1] == 6:
        if not np.all(s[:, 3] == 1.0):
            raise ValueError("sos [K, 6]: a0 must be 1 in every section")
        s = np.delete(s, 3, axis=1)
    if not 1 <= s.shape[0] <= MAX_SECTIONS:
        raise ValueError(f"1 .. {MAX_SECTIONS} sections, got {s.shape[0]}")
    if not np.all(np.isfinite(s)):
        raise ValueError("sos: every coefficient must be finite")
    for q, (_, _, _, a1, a2) in enumerate(s):
        if not (abs(a2) < 1.0 and abs(a1) < 1.0 + a2):
            raise ValueError(f"section {q} has a pole on or outside the unit circle: |a2| < 1 and |a1| < 1 + a2 are required, got a1 {a1!r}, a2 {a2!r}")
    return np.ascontiguousarray(s)


def _coefficient(coef, name: str) -> float:
    if isinstance(coef, bool) or not isinstance(coef, (int, float, np.integer, np.floating)) or not 0.0 <= float(coef) < 1.0:
        raise ValueError(f"{name} must be a number in [0, 1), got {coef!r}")
    return float(coef)


def preemphasis_sos(coef: float) -> np.ndarray:
    """[1, 5]: y[n] = x[n] - coef x[n - 1]"""
    return np.array([[1.0, -_coefficient(coef, "preemphasis"), 0.0, 0.0, 0.0]])


def deemphasis_sos(coef: float) -> np.ndarray:
    """[1, 5]: y[n] = x[n] + coef y[n - 1], the inverse of `preemphasis_sos(coef)`"""
    return np.array([[1.0, 0.0, 0.0, -_coefficient(coef, "deemphasis"), 0.0]])


def highpass_sos(sampling_rate, cutoff_hz, order: int = 2) -> np.ndarray:
    """[order / 2, 5]: the Butterworth high-pass of that order with its -3.01 dB point at `cutoff_hz`, by the bilinear transform with
    pre-warping, in float64.  With k = tan(pi cutoff / rate) and the section's Q (order 2: 1 / sqrt 2; order 4: 1 / (2 cos(pi / 8)) and
    1 / (2 cos(3 pi / 8))):  b = (1, -2, 1) / n,  a1 = 2 (k^2 - 1) / n,  a2 = (1 - k / Q + k^2) / n,  n = 1 + k / Q + k^2."""
    if isinstance(sampling_rate, bool) or not isinstance(sampling_rate, (int, float, np.integer, np.floating)) or not float(sampling_rate) > 0.0:
        raise ValueError(f"sampling_rate must be a positive number, got {sampling_rate!r}")
    if isinstance(order, bool) or order not in (2, 4):
        raise ValueError(f"highpass order must be 2 or 4, got {order!r}")
    fs = float(sampling_rate)
    if isinstance(cutoff_hz, bool) or not isinstance(cutoff_hz, (int, float, np.integer, np.floating)) or not 0.0 < float(cutoff_hz) < fs / 2.0:
        raise ValueError(f"highpass cutoff must lie inside (0, {fs / 2.0}) Hz, got {cutoff_hz!r}")
    k = math.tan(math.pi * float(cutoff_hz) / fs)
    qs = [1.0 / math.sqrt(2.0)] if order == 2 else [1.0 / (2.0 * math.cos(math.pi / 8.0)), 1.0 / (2.0 * math.cos(3.0 * math.pi / 8.0))]
    out = []
    for q in qs:
        n = 1.0 + k / q + k * k
        out.append([1.0 / n, -2.0 / n, 1.0 / n, 2.0 * (k * k - 1.0) / n, (1.0 - k / q + k * k) / n])
    return np.array(out, dtype=np.float64)


# ---------------------------------------------------------------------------------------------- state carry
def transition_powers(sos: np.ndarray, segment: int = SEGMENT, steps: int = SCAN_STEPS) -> np.ndarray:
    """float64 [steps, 2K, 2K]: M^(2^k) for k = 0 .. steps - 1, M being the map of the cascade's state (s1, s2 of every section in order) over
    `segment` samples of zero input.  Column i of entry k is the state after 2^k `segment` zero-input steps of the recurrence from the unit
    state e_i: the recurrence itself is run, all 2K unit states side by side, and read off at those counts."""
    sos = np.asarray(sos, dtype=np.float64)
    K = sos.shape[0]
    N = 2 * K
    s = np.eye(N, dtype=np.float64)                           # s[:, i]: the state that began as e_i
    out = np.empty((steps, N, N), dtype=np.float64)
    mark, k = segment, 0
    for n in range(1, segment * 2 ** (steps - 1) + 1):
        x = np.zeros(N, dtype=np.float64)
        for q in range(K):
            b0, b1, b2, a1, a2 = sos[q]
            y = b0 * x + s[2 * q]
            s[2 * q] = b1 * x - a1 * y + s[2 * q + 1]
            s[2 * q + 1] = b2 * x - a2 * y
            x = y
        if n == mark:
            out[k] = s
            mark, k = 2 * mark, k + 1
    return out


_POWERS = {}             # sos bytes -> transition_powers(sos): built once per filter


def cached_powers(sos: np.ndarray) -> np.ndarray:
    key = sos.tobytes()
    if key not in _POWERS:
        _POWERS[key] = transition_powers(sos)
    return _POWERS[key]


class IIRFilter(torch.nn.Module):
    """out = IIRFilter(device, sos)(audio [B, n] float32 | int16, lengths=None)

    out: fp32 [B, n], every item run through the cascade `sos` ([K, 5] rows (b0, b1, b2, a1, a2), or scipy's [K, 6] with a0 == 1; K <= 4) from
    zero state at its first sample, in fp64 and rounded once; zero behind its length.  int16 PCM is taken as x / max_wav_value.  Every item
    is treated exactly as if it had been passed alone.  Lengths do not change.  A section with a pole on or outside the unit circle is
    refused."""

    def __init__(self, device=None, sos=None, max_wav_value: float = 32768.0):
        super().__init__()
        if sos is None:
            raise ValueError("IIRFilter needs its sections: sos [K, 5] or [K, 6]")
        self.dev = None if device is None else torch.device(device)
        self.max_wav_value = A.max_wav(max_wav_value)
        self.sos = check_sos(sos)
        self.sections = int(self.sos.shape[0])
        self.powers = cached_powers(self.sos)
        self._sos = (ctypes.c_double * self.sos.size)(*self.sos.reshape(-1).tolist())
        self._powers = A.Cache(capacity=5)   # device -> the matrices there
        self._ws = A.Cache(capacity=5)       # (device, B, n) -> workspace

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        audio = A.signal(audio, "audio", "IIRFilter")
        B, n = audio.shape
        lib = L_.load()
        L_.require_device()
        dev = audio.device
        li = A.device_lengths(lengths, B, n, dev)
        ws = self._ws.get((dev, B, n), lambda: torch.empty(max(int(lib.efts_iir_workspace_bytes(B, n)), 16), dtype=torch.uint8, device=dev))
        powers = self._powers.get(dev, lambda: torch.from_numpy(self.powers).to(dev).contiguous())
        out = torch.empty(B, n, dtype=torch.float32, device=dev)
        fn, name, scale = A.pcm_entry(lib, "efts_iir", audio, self.max_wav_value)
        with O.stream_scope():
            L_.check(fn(audio.data_ptr(), n, li.data_ptr(), self._sos, self.sections, powers.data_ptr(), *scale, out.data_ptr(), n, ws.data_ptr(), B, O._stream()), name)
        return out


def build_chain(device, sampling_rate, highpass_hz=None, highpass_order=None, deemphasis=None, max_wav_value: float = 32768.0) -> Optional[IIRFilter]:
    """the one IIRFilter that a command line asks for: the high-pass first, de-emphasis behind it; None when neither is given.  Every value
    out of range is refused, and so is an order without a cutoff."""
    if highpass_hz is None and highpass_order is not None:
        raise ValueError("highpass_order: set without highpass_hz")
    parts = []
    if highpass_hz is not None:
        parts.append(highpass_sos(sampling_rate, highpass_hz, 2 if highpass_order is None else highpass_order))
    if deemphasis is not None:
        parts.append(deemphasis_sos(deemphasis))
    if not parts:
        return None
    return IIRFilter(device, np.concatenate(parts, axis=0), max_wav_value=max_wav_value)
