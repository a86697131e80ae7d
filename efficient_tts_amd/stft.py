"""On-device STFT magnitudes at several resolutions and the multi-resolution STFT distance between two signals: the measure that
copy-synthesis (recording -> log-mel -> vocoder -> audio) is judged by, `MultiResolutionSTFTLoss` of nntts/losses/stft_loss.py without its
backward pass.

One resolution is (N, H, W): FFT size N in {256, 512, 1024, 2048}, hop 1 <= H <= N, window length 2 <= W <= N.  With x the candidate and
y the reference signal, per item of L samples:

    window   periodic Hann of length W, float64 on the host, rounded once to fp32, (N - W) // 2 zeros in front of it in the frame
    frames   T = 1 + L // H, centred, N / 2 samples of reflect padding at both ends; L <= N / 2: no frames
    mag      sqrt(max(re^2 + im^2, 1e-7)) for f = 0 .. N / 2
    num = sum (mag_y - mag_x)^2,  den = sum mag_y^2,  l1 = sum |ln mag_y - ln mag_x|   over the item's own T (N / 2 + 1) cells
    sc = sqrt(num) / sqrt(den),  log_mag = l1 / (T (N / 2 + 1));  no frames: cells = 0 and NaN

include/efts_abi.h has the full definition, summation order included.  The sums run in csrc/efts_stft.hip (`efts_stft_mag`, `efts_stft_dist`):
one launch per resolution plus a small one that adds the frames in float64; no spectrogram goes to memory on the distance path, no atomics,
nothing read back by the host.  No CPU path: the HIP library is required.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import audio_args as A
from . import lib as L_
from . import ops as O

FFT_SIZES = (256, 512, 1024, 2048)
DEFAULT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))      # stft_loss.py:113-116


def check_resolution(n_fft, hop_size, win_length) -> Tuple[int, int, int]:
    n, h, w = A.as_int(n_fft, "n_fft"), A.as_int(hop_size, "hop_size"), A.as_int(win_length, "win_length")
    if n not in FFT_SIZES:
        raise ValueError(f"n_fft must be one of {FFT_SIZES}, got {n_fft!r}")
    if not 1 <= h <= n:
        raise ValueError(f"hop_size must lie in 1 .. n_fft, got {hop_size!r}")
    if not 2 <= w <= n:
        raise ValueError(f"win_length must lie in 2 .. n_fft, got {win_length!r}")
    return n, h, w


def hann_window(win_length: int) -> np.ndarray:
    """the periodic Hann window of torch.hann_window(win_length): float64, rounded once to fp32"""
    i = np.arange(win_length, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / win_length)).astype(np.float32)


def frame_count(length: int, n_fft: int, hop_size: int) -> int:
    """frames of an item of `length` samples: 1 + length // hop, or 0 when it is too short for the reflect padding"""
    return 1 + length // hop_size if length > n_fft // 2 else 0


class STFTMagnitude(torch.nn.Module):
    """mag, frames = STFTMagnitude(device, n_fft, hop_size, win_length)(audio [B, n] float32 | int16, lengths=None)

    mag: fp32 [B, 1 + n // hop_size, n_fft // 2 + 1], zero at and beyond an item's frame count; frames: int64 [B] (0 for an item of at most
    n_fft / 2 samples)."""

    def __init__(self, device=None, n_fft: int = 1024, hop_size: int = 120, win_length: int = 600, max_wav_value: float = 32768.0):
        super().__init__()
        self.dev = None if device is None else torch.device(device)
        self.n_fft, self.hop, self.win_length = check_resolution(n_fft, hop_size, win_length)
        self.max_wav_value = A.max_wav(max_wav_value)
        self._window = {}                # device -> window

    def _win(self, dev) -> torch.Tensor:
        if dev not in self._window:
            self._window[dev] = torch.from_numpy(hann_window(self.win_length)).to(dev)
        return self._window[dev]

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        audio = A.signal(audio, "audio", "efficient_tts_amd.stft")
        B, n = audio.shape
        lib = L_.load()
        L_.require_device()
        dev = audio.device
        li = A.device_lengths(lengths, B, n, dev)
        T = 1 + n // self.hop
        mag = torch.empty(B, T, self.n_fft // 2 + 1, dtype=torch.float32, device=dev)
        frames = torch.empty(B, dtype=torch.int32, device=dev)
        with O.stream_scope():
            L_.check(lib.efts_stft_mag(audio.data_ptr(), int(audio.dtype == torch.int16), 1.0 / self.max_wav_value, n, li.data_ptr(), n,
                                       self._win(dev).data_ptr(), mag.data_ptr(), frames.data_ptr(), B, self.n_fft, self.hop, self.win_length,
                                       O._stream()), "efts_stft_mag")
        return mag, frames.to(torch.int64)


class MultiResolutionSTFTDistance(torch.nn.Module):
    """out = MultiResolutionSTFTDistance(device, resolutions, max_wav_value)(x, y, lengths=None)

    x (the candidate) and y (the reference): [B, n] and [B, m], float32 or int16 independently of each other; item b is compared over
    lengths[b] samples (default min(n, m)).  out: sc [B, R] and log_mag [B, R] (float64; NaN where an item is too short for a resolution),
    sums [B, R, 3] (float64: num, den, l1) and cells [B, R] (int64).  Every item is scored exactly as if it had been passed alone, and
    nothing is read back by the host.  `batch_loss(out)` reduces them the way the reference's loss reduces a batch."""

    def __init__(self, device=None, resolutions: Sequence[Sequence[int]] = DEFAULT_RESOLUTIONS, max_wav_value: float = 32768.0):
        super().__init__()
        self.dev = None if device is None else torch.device(device)
        self.resolutions = tuple(check_resolution(*r) for r in resolutions)
        if not self.resolutions:
            raise ValueError("at least one resolution")
        self.max_wav_value = A.max_wav(max_wav_value)
        self._window = {}                # (device, W) -> window
        self._ws = A.Cache(capacity=5)   # (device, B, n) -> one workspace, large enough for every resolution

    def _win(self, dev, w: int) -> torch.Tensor:
        if (dev, w) not in self._window:
            self._window[(dev, w)] = torch.from_numpy(hann_window(w)).to(dev)
        return self._window[(dev, w)]

    @torch.no_grad()
    def forward(self, x: torch.Tensor, y: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        x, y = A.signal(x, "x", "efficient_tts_amd.stft"), A.signal(y, "y", "efficient_tts_amd.stft")
        if x.shape[0] != y.shape[0] or x.device != y.device:
            raise ValueError("x and y must hold the same number of items on the same device")
        B, n = x.shape[0], min(x.shape[1], y.shape[1])
        lib = L_.load()
        L_.require_device()
        dev = x.device
        li = A.device_lengths(lengths, B, n, dev)
        R = len(self.resolutions)
        sums = torch.empty(R, B, 3, dtype=torch.float64, device=dev)
        cells = torch.empty(R, B, dtype=torch.int64, device=dev)
        ws = self._ws.get((dev, B, n), lambda: torch.empty(max(int(lib.efts_stft_dist_workspace_bytes(B, n, N, H)) for N, H, _ in self.resolutions),
                                                           dtype=torch.uint8, device=dev))
        with O.stream_scope():
            for r, (N, H, W) in enumerate(self.resolutions):
                L_.check(lib.efts_stft_dist(x.data_ptr(), int(x.dtype == torch.int16), x.shape[1], y.data_ptr(), int(y.dtype == torch.int16), y.shape[1],
                                            1.0 / self.max_wav_value, li.data_ptr(), n, self._win(dev, W).data_ptr(), sums[r].data_ptr(),
                                            cells[r].data_ptr(), ws.data_ptr(), ws.numel(), B, N, H, W, O._stream()), "efts_stft_dist")
        sums, cells = sums.transpose(0, 1).contiguous(), cells.transpose(0, 1).contiguous()
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        has = cells > 0
        sc = torch.where(has, sums[..., 0].sqrt() / sums[..., 1].sqrt(), nan)
        log_mag = torch.where(has, sums[..., 2] / cells.clamp(min=1).to(torch.float64), nan)
        return {"sc": sc, "log_mag": log_mag, "sums": sums, "cells": cells}

    @staticmethod
    def batch_loss(out) -> Tuple[torch.Tensor, torch.Tensor]:
        """(sc_loss, mag_loss) of MultiResolutionSTFTLoss.forward (stft_loss.py:133-156) from the per-item sums: per resolution the Frobenius
        norms over the whole batch and the mean over all its cells, then the mean over the resolutions.  Equal to the reference's value for
        a batch of equal lengths, where its spectrograms hold exactly the items' own cells."""
        sums, cells = out["sums"], out["cells"]
        tot = sums.sum(dim=0)                                              # [R, 3]
        sc = tot[:, 0].sqrt() / tot[:, 1].sqrt()
        mag = tot[:, 2] / cells.sum(dim=0).to(torch.float64)
        return sc.mean(), mag.mean()
