"""On-device true-peak metering after ITU-R BS.1770 Annex 2 / EBU R 128 of a padded batch, and a look-ahead peak limiter that holds every
item under a true-peak ceiling: the peak half of the standard whose loudness half is `efficient_tts_amd.loudness`.  At synthesis the limiter
is the last step in front of the 16-bit quantisation, so that a loudness target can be reached and the peaks are taken where they stand.

With x = 0 outside an item's [0, len), h = `true_peak_table()` (4 phases, 25 taps) and the ceiling c:

    xo[i][q] = sum over k = -12 .. 12 of x[i + k] h[q][k + 12]       the signal at i + q / 4; phase 0 is the sample itself
    p[i] = max over q of |xo[i][q]|;  true peak = max p[i],  sample peak = max |x[i]|
    r[i] = c / p[i] if p[i] > c, else 1                                the gain that sample i needs; 1 outside the item
    m[i] = min of r[j] over |j - i| <= H                              held for H samples on either side
    g[i] = min(r[i], mean of m[j] over |j - i| <= S)                  the box of 2 S + 1 samples smooths the steps of m;  S <= H
    out[i] = x[i] g[i] for i < len, 0 behind

include/efts_abi.h has the definition to the bit, summation orders included.  The sums run in csrc/efts_limiter.hip (`efts_true_peak`,
`efts_peak_limit` and their `_pcm16` twins): two launches per call, no atomics, nothing read back by the host.  The limiter works offline and
symmetrically (it looks H + S samples ahead and as many back), the oversampling is 4x only, H <= 128, and there is no release curve beyond
the box.  No CPU path: the HIP library is required.
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

PHASES, ZEROS, BETA = 4, 12, 8.0
TAPS = 2 * ZEROS + 1
MAX_HOLD = 128


def true_peak_table() -> np.ndarray:
    """float32 [4, 25]: h[q][k + 12] = sinc(t) I0(8 sqrt(1 - (t / 12)^2)) / I0(8) with t = q / 4 - k, 0 for |t| >= 12; float64, rounded once.
    sinc of a non-zero integer is exactly 0, so phase 0 is the identity to the bit."""
    q = np.arange(PHASES, dtype=np.float64)[:, None]
    k = np.arange(-ZEROS, ZEROS + 1, dtype=np.float64)[None, :]
    t = q / PHASES - k
    inside = np.abs(t) < ZEROS
    window = np.i0(BETA * np.sqrt(np.where(inside, 1.0 - (t / ZEROS) ** 2, 0.0))) / np.i0(BETA)
    whole = t == np.round(t)
    sinc = np.where(whole, (t == 0.0).astype(np.float64), np.sin(np.pi * t) / np.where(whole, 1.0, np.pi * t))
    return np.where(inside, sinc * window, 0.0).astype(np.float32)


def lookahead_samples(lookahead_ms: float, sampling_rate: int) -> int:
    return int(round(float(lookahead_ms) * sampling_rate / 1000.0))


class _Peaks(torch.nn.Module):
    """what the meter and the limiter share: the table, the workspace and the argument checks"""

    def __init__(self, device, max_wav_value: float):
        super().__init__()
        self.dev = None if device is None else torch.device(device)
        self.max_wav_value = A.max_wav(max_wav_value)
        self.table = true_peak_table()
        self._table = (ctypes.c_float * (PHASES * TAPS))(*self.table.reshape(-1).tolist())
        self._ws = A.Cache(capacity=5)   # (device, B, n) -> workspace

    def _prepare(self, who: str, audio: torch.Tensor, lengths: Optional[torch.Tensor]):
        audio = A.signal(audio, "audio", who)
        B, n = audio.shape
        lib = L_.load()
        L_.require_device()
        dev = audio.device
        li = A.device_lengths(lengths, B, n, dev)
        ws = self._ws.get((dev, B, n), lambda: torch.empty(max(int(lib.efts_limiter_workspace_bytes(B, n)), 16), dtype=torch.uint8, device=dev))
        return lib, audio, li, ws


class TruePeakMeter(_Peaks):
    """true_peak, sample_peak = TruePeakMeter(device)(audio [B, n] float32 | int16, lengths=None)

    Both fp32 [B], linear (20 log10 of the first is dBTP): the largest magnitude of the 4x oversampled signal and of the samples, 0 for an
    empty item; true_peak >= sample_peak always.  int16 PCM is taken as x / max_wav_value.  Every item is treated exactly as if it had been
    passed alone."""

    def __init__(self, device=None, max_wav_value: float = 32768.0):
        super().__init__(device, max_wav_value)

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        lib, audio, li, ws = self._prepare("TruePeakMeter", audio, lengths)
        B, n = audio.shape
        true_peak = torch.empty(B, dtype=torch.float32, device=audio.device)
        sample_peak = torch.empty(B, dtype=torch.float32, device=audio.device)
        fn, name, scale = A.pcm_entry(lib, "efts_true_peak", audio, self.max_wav_value)
        with O.stream_scope():
            L_.check(fn(audio.data_ptr(), n, li.data_ptr(), self._table, *scale, true_peak.data_ptr(), sample_peak.data_ptr(), ws.data_ptr(), B,
                        O._stream()), name)
        return true_peak, sample_peak


class PeakLimiter(_Peaks):
    """out = PeakLimiter(device, sampling_rate, ceiling_dbtp, lookahead_ms, hold, smooth)(audio [B, n] float32 | int16, lengths=None)

    out: fp32 [B, n], every item multiplied by a gain curve that keeps its samples, and as far as the curve is smooth its true peak, under
    10^(ceiling_dbtp / 20); zero behind its length.  The curve reaches what a peak needs `hold` samples before it and leaves it `hold`
    samples after it, smoothed by a box of 2 `smooth` + 1 samples; both default to `lookahead_ms` at the sampling rate and must satisfy
    1 <= smooth <= hold <= 128.  An item whose true peak is not above the ceiling comes back bit for bit.  With `return_stats=True` also
    gain_min fp32 [B] (the smallest gain applied), limited int32 [B] (samples with a gain below 1) and true_peak_in fp32 [B] (the true peak
    of the input).  Lengths do not change."""

    def __init__(self, device=None, sampling_rate: int = 22050, ceiling_dbtp: float = -1.0, lookahead_ms: float = 1.5, hold: Optional[int] = None,
                 smooth: Optional[int] = None, max_wav_value: float = 32768.0):
        super().__init__(device, max_wav_value)
        self.sampling_rate = A.as_int(sampling_rate, "sampling_rate")
        if self.sampling_rate < 1:
            raise ValueError(f"sampling_rate must be positive, got {sampling_rate!r}")
        self.ceiling_dbtp = float(ceiling_dbtp)
        if not math.isfinite(self.ceiling_dbtp) or self.ceiling_dbtp > 0.0:
            raise ValueError(f"ceiling_dbtp must be a finite level of at most 0 dBTP, got {ceiling_dbtp!r}")
        self.ceiling = float(np.float32(10.0 ** (self.ceiling_dbtp / 20.0)))          # what the kernel compares with, by value
        if not (float(lookahead_ms) > 0.0 and math.isfinite(float(lookahead_ms))):
            raise ValueError(f"lookahead_ms must be a positive number, got {lookahead_ms!r}")
        default = lookahead_samples(lookahead_ms, self.sampling_rate)
        self.hold = default if hold is None else A.as_int(hold, "hold")
        self.smooth = min(default, self.hold) if smooth is None else A.as_int(smooth, "smooth")
        if not 1 <= self.smooth <= self.hold <= MAX_HOLD:
            raise ValueError(f"1 <= smooth <= hold <= {MAX_HOLD} is required, got hold {self.hold} and smooth {self.smooth} "
                             f"(lookahead_ms {lookahead_ms!r} at {self.sampling_rate} Hz is {default} samples)")

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None, return_stats: bool = False):
        lib, audio, li, ws = self._prepare("PeakLimiter", audio, lengths)
        B, n = audio.shape
        dev = audio.device
        out = torch.empty(B, n, dtype=torch.float32, device=dev)
        gain_min = torch.empty(B, dtype=torch.float32, device=dev)
        limited = torch.empty(B, dtype=torch.int32, device=dev)
        true_peak_in = torch.empty(B, dtype=torch.float32, device=dev)
        fn, name, scale = A.pcm_entry(lib, "efts_peak_limit", audio, self.max_wav_value)
        with O.stream_scope():
            L_.check(fn(audio.data_ptr(), n, li.data_ptr(), self._table, *scale, self.ceiling, self.hold, self.smooth, out.data_ptr(), n,
                        gain_min.data_ptr(), limited.data_ptr(), true_peak_in.data_ptr(), ws.data_ptr(), B, O._stream()), name)
        if return_stats:
            return out, gain_min, limited, true_peak_in
        return out
