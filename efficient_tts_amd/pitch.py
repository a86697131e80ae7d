"""On-device pitch tracking: YIN (de Cheveigne & Kawahara 2002) on the frame grid of `LogMelFrontend`, so that f0[b, t] belongs to mel[b, t].

Item b has lengths[b] // hop frames; frame t covers samples t hop - pad .. t hop - pad + n_fft - 1 with pad = (n_fft - hop) / 2, reflected at
the item's ends.  Per frame x, with W = n_fft / 2, tau_min = floor(sr / fmax) and tau_max = floor(sr / fmin) <= W:

    d(tau)  = sum_{j < W} (x[j] - x[j + tau])^2                       (the direct form, fp32 fused multiply-adds, j ascending)
    d'(tau) = d(tau) tau / (d(1) + .. + d(tau)), 1 where that sum is 0
    tau     = the smallest lag in [tau_min, tau_max - 1] with d'(tau) < threshold, advanced while d' keeps falling, refined by a parabola
              through d'(tau - 1), d'(tau), d'(tau + 1) (shift clamped to [-1, 1]);  f0 = sr / tau, or 0 when no lag is under the threshold

One launch (csrc/efts_pitch.hip, `efts_yin` / `efts_yin_pcm16`); include/efts_abi.h states every order of summation.  fp32, no atomics: an
item gives the same bits alone, in any batch position and in any run.  No smoothing across frames (no pYIN / Viterbi).  No CPU path: the
HIP library is required.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import lib as L
from . import ops as O

N_FFTS = (512, 1024, 2048)


def lag_range(sampling_rate: int, n_fft: int, fmin: float, fmax: float):
    """(tau_min, tau_max) as the library computes them -- floor(sr / fmax), floor(sr / fmin) in float64 on the fp32 values of fmin and fmax --
    or ValueError where the library would refuse"""
    lo = math.floor(sampling_rate / float(np.float32(fmax))) if fmax > 0 else 0
    hi = math.floor(sampling_rate / float(np.float32(fmin))) if fmin > 0 else 0
    if not (fmin > 0 and fmax > fmin and lo >= 2 and hi <= n_fft // 2 and lo < hi - 1):
        raise ValueError(f"need 0 < fmin < fmax with 2 <= floor(sr / fmax) < floor(sr / fmin) - 1 and floor(sr / fmin) <= n_fft / 2; "
                         f"got lags {lo} .. {hi} for n_fft {n_fft} (fmin {fmin}, fmax {fmax}, sr {sampling_rate})")
    return lo, hi


class PitchTracker:
    """f0, aperiodicity, frames = PitchTracker(device)(audio, lengths)

    audio: [B, L] float32 in [-1, 1] or int16 PCM (scaled by 1 / max_wav_value at the kernel's loads), on the device or the host; lengths: [B]
    sample counts.  Returns f0 [B, T] in Hz (0: unvoiced, and frames at or beyond an item's count), aperiodicity [B, T] (d' at the chosen
    lag, or its minimum over the search range for an unvoiced frame: apply a threshold of your own to it) and frames [B] int64;
    T = max frames or `max_frames`.  `return_cmnd=True` appends cmnd [B, T, tau_max + 1], every d'(tau).  `short_ok=True` gives an item no
    longer than the reflect padding zero frames instead of refusing it."""

    def __init__(self, device, sampling_rate: int = 22050, n_fft: int = 1024, hop_size: int = 256, fmin: float = 60.0, fmax: float = 600.0,
                 threshold: float = 0.15, max_wav_value: float = 32768.0):
        if n_fft not in N_FFTS:
            raise ValueError(f"n_fft must be one of {N_FFTS}")
        if not 1 <= hop_size <= n_fft or (n_fft - hop_size) % 2:
            raise ValueError("hop_size must lie in 1 .. n_fft with n_fft - hop_size even")
        if not threshold > 0 or not max_wav_value > 0:
            raise ValueError("threshold and max_wav_value must be > 0")
        self.tau_min, self.tau_max = lag_range(int(sampling_rate), n_fft, fmin, fmax)
        self.dev = torch.device(device)
        self.sr, self.n_fft, self.hop, self.pad = int(sampling_rate), int(n_fft), int(hop_size), (n_fft - hop_size) // 2
        self.fmin, self.fmax, self.threshold, self.max_wav_value = float(fmin), float(fmax), float(threshold), float(max_wav_value)
        L.load()
        L.require_device()

    def frames_of(self, lengths: torch.Tensor) -> torch.Tensor:
        return torch.div(lengths.to(torch.int64), self.hop, rounding_mode="floor")

    @torch.no_grad()
    def __call__(self, audio: torch.Tensor, lengths: torch.Tensor, max_frames: Optional[int] = None, return_cmnd: bool = False, short_ok: bool = False):
        if audio.dim() != 2 or audio.dtype not in (torch.float32, torch.int16):
            raise ValueError("audio must be [B, L], float32 or int16")
        B = audio.shape[0]
        if lengths.shape != (B,):
            raise ValueError("lengths must be [B]")
        audio = audio.to(self.dev).contiguous()
        lh = lengths.detach().to("cpu", torch.int64).tolist()                       # the one host copy: the checks run on plain ints
        if max(lh) > audio.shape[1]:
            raise ValueError("lengths exceed the audio buffer")
        if min(lh) <= self.pad and not short_ok:
            raise ValueError("every item must be longer than the reflect padding (n_fft - hop) / 2")
        fh = [l // self.hop if l > self.pad else 0 for l in lh]
        T = max(max(fh), 1) if max_frames is None else int(max_frames)
        if T < 1:
            raise ValueError("max_frames must be >= 1")
        both = torch.tensor([lh, fh], dtype=torch.int32).to(self.dev, non_blocking=True)
        f0 = torch.empty(B, T, dtype=torch.float32, device=self.dev)
        ap = torch.empty(B, T, dtype=torch.float32, device=self.dev)
        cmnd = torch.empty(B, T, self.tau_max + 1, dtype=torch.float32, device=self.dev) if return_cmnd else None
        lib = L.load()
        tail = (f0.data_ptr(), ap.data_ptr(), O._p(cmnd), B, T, self.n_fft, self.hop, self.sr, self.fmin, self.fmax, self.threshold)
        with O.stream_scope():
            if audio.dtype == torch.int16:
                L.check(lib.efts_yin_pcm16(audio.data_ptr(), audio.shape[1], 1.0 / self.max_wav_value, both[0].data_ptr(), *tail, O._stream()), "efts_yin_pcm16")
            else:
                L.check(lib.efts_yin(audio.data_ptr(), audio.shape[1], both[0].data_ptr(), *tail, O._stream()), "efts_yin")
        frames = both[1].to(torch.int64)
        return (f0, ap, frames, cmnd) if return_cmnd else (f0, ap, frames)
