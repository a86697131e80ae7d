"""On-device short-time objective intelligibility of a processed signal against the clean one: STOI (Taal et al. 2011) and its extended form
ESTOI (Jensen and Taal 2016), the standard numbers for "does the speech stay intelligible", as the authors' Matlab code (and pystoi after it)
computes them.  Both signals are time-aligned, which is what copy-synthesis produces, and are compared at 10 000 Hz over n samples:

    frames   256 samples, hop 128, w = numpy's hanning(258)[1:-1];  F = (n - 256) // 128 + 1 when n >= 256, otherwise 0
    silence  a frame of x is kept iff its energy times 10^4 exceeds the largest frame energy of x (40 dB); the same frames are kept from y
    spectra  the kept windowed frames are overlap-added, framed again (all but the last: T = K - 1), 512-point DFT, |.|^2 summed over 15
             one-third-octave bands from 150 Hz, square root
    segments of 30 frames, M = T - 29:  STOI: per band, y scaled to x's norm and clipped at x (1 + 10^(15/20)), then the correlation
             coefficient of the two rows; the mean over bands and segments.  ESTOI: rows, then columns, made zero-mean and unit-norm; the
             mean over frames and segments of the columns' inner products

include/efts_abi.h has the full definition, the order of every sum included; tests/stoi_reference.py restates it in numpy float64.  It runs
in csrc/efts_stoi.hip (`efts_stoi`): fp32 transforms and band sums, float64 segments, no atomics, nothing read back by the host.  An item
without a segment (fewer than 256 samples, at most 30 kept frames, an all-zero x) scores NaN, where the reference code warns and returns
1e-5.  No CPU path: the HIP library is required.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import audio_args as A
from . import lib as L_
from . import ops as O
from .resample import Resampler

FS, FRAME, HOP, N_FFT, BANDS, SEGMENT = 10000, 256, 128, 512, 15, 30


def stoi_window() -> np.ndarray:
    """w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), float64 on the host, rounded once to fp32"""
    i = np.arange(FRAME, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 1.0) / (FRAME + 1.0))).astype(np.float32)


def _pair(x: torch.Tensor, y: torch.Tensor):
    """x and y after the checks of two padded batches that belong together: shapes and types first, then the device"""
    x, y = A.signal(x, "x"), A.signal(y, "y")
    if x.shape[0] != y.shape[0]:
        raise ValueError("x and y must hold the same number of items")
    x, y = A.signal(x, "x", "ShortTimeIntelligibility"), A.signal(y, "y", "ShortTimeIntelligibility")
    if x.device != y.device:
        raise ValueError("x and y must be on the same device")
    return x, y


class ShortTimeIntelligibility(torch.nn.Module):
    """out = ShortTimeIntelligibility(device, sampling_rate=22050, quality="best")(x [B, n], y [B, m], lengths=None)

    x: the clean signal, y: the processed one, each float32 or int16 (scaled by 1 / max_wav_value) at `sampling_rate`; they are compared
    over lengths [B] samples (default min(n, m)).  With sampling_rate != 10000 both pass through one `Resampler(sampling_rate, 10000,
    quality)` first.  out: dict with stoi, estoi float64 [B] (NaN for an item without a segment) and frames, kept, segments int64 [B]: the
    frames at 10 kHz, those kept after silent-frame removal and the 30-frame segments scored.  Every item is scored exactly as if it had been
    passed alone."""

    def __init__(self, device=None, sampling_rate: int = 22050, quality: str = "best", max_wav_value: float = 32768.0):
        super().__init__()
        self.dev = None if device is None else torch.device(device)
        self.max_wav_value = A.max_wav(max_wav_value)
        self.resampler = Resampler(device, sampling_rate, FS, quality, max_wav_value=self.max_wav_value)    # (checks the rate and the quality)
        self.sampling_rate = self.resampler.src_rate
        self._windows = {}               # device -> window
        self._ws = A.Cache(capacity=5)   # (device, B, n) -> workspace

    def _window(self, dev) -> torch.Tensor:
        if dev not in self._windows:
            self._windows[dev] = torch.from_numpy(stoi_window()).to(dev)
        return self._windows[dev]

    @torch.no_grad()
    def forward(self, x: torch.Tensor, y: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        x, y = _pair(x, y)
        B, dev = x.shape[0], x.device
        li = A.device_lengths(lengths, B, min(x.shape[1], y.shape[1]), dev)
        x10, n10 = self.resampler(x, li)
        y10, _ = self.resampler(y, li)
        return self.score_10k(x10, y10, n10)

    @torch.no_grad()
    def score_10k(self, x: torch.Tensor, y: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """the core call: x, y float32 at 10 000 Hz"""
        if x.dtype != torch.float32 or y.dtype != torch.float32:
            raise ValueError("score_10k takes float32 samples at 10 000 Hz")
        x, y = _pair(x, y)
        B, dev = x.shape[0], x.device
        n = min(x.shape[1], y.shape[1])
        lib = L_.load()
        L_.require_device()
        li = A.device_lengths(lengths, B, n, dev)
        window = self._window(dev)
        scores = torch.empty(2, B, dtype=torch.float64, device=dev)
        counts = torch.empty(3, B, dtype=torch.int32, device=dev)
        nbytes = int(lib.efts_stoi_workspace_bytes(B, n))
        ws = self._ws.get((dev, B, n), lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
        with O.stream_scope():
            L_.check(lib.efts_stoi(x.data_ptr(), x.shape[1], y.data_ptr(), y.shape[1], li.data_ptr(), n, window.data_ptr(), scores[0].data_ptr(),
                                   scores[1].data_ptr(), counts[0].data_ptr(), counts[1].data_ptr(), counts[2].data_ptr(), ws.data_ptr(), nbytes, B,
                                   O._stream()), "efts_stoi")
        counts = counts.to(torch.int64)
        return dict(stoi=scores[0], estoi=scores[1], frames=counts[0], kept=counts[1], segments=counts[2])
