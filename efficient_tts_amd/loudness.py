"""On-device integrated loudness after ITU-R BS.1770 / EBU R 128 of a padded batch of recordings, and normalisation to a target loudness:
what `pyloudnorm` / `ffmpeg loudnorm` do offline, as one step of the device-side data path (behind `SilenceTrimmer`, in front of
`LogMelFrontend`) and behind the vocoder at synthesis.

With h = sampling_rate / 10 and x = 0 outside an item's [0, len):

    y = HP(SHELF(x))                      the K-weighting filter, two biquads, fp64 (`k_weighting` has the coefficients)
    z_j = sum of y^2 over samples j h .. j h + 4 h - 1, / (4 h)      j = 0 .. floor(len / h) - 4: 400 ms blocks at a 100 ms hop
    A = { j : z_j > 10^((-70 + 0.691) / 10) },  G = { j in A : z_j > 0.1 mean(z_j, j in A) }
    L = -0.691 + 10 log10(mean(z_j, j in G))                         no block, or A empty: L = -inf, flag bit 0
    g = 10^((target - L) / 20);  with a ceiling and g max |x| > ceiling: g = ceiling / max |x|, flag bit 1;  L = -inf: g = 1
    out[i] = x[i] * g for i < len, 0 behind                          (int16 PCM: g includes 1 / max_wav_value)

include/efts_abi.h has the full definition, summation orders and the way the recurrence is cut into parallel segments included.  The sums
run in csrc/efts_loudness.hip (`efts_loudness`, `efts_loudness_pcm16`): three launches (two when only measuring), no atomics, nothing read
back by the host.  No CPU path: the HIP library is required.
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

MIN_RATE, MAX_RATE = 8000, 48000
FLAG_NO_LOUDNESS, FLAG_CEILING = 1, 2


def k_weighting(sampling_rate: int) -> np.ndarray:
    """float64 [10]: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 (a0 = 1) -- the bilinear designs of libebur128, which reproduce the
    table of BS.1770 at 48 kHz"""
    fs = float(sampling_rate)
    K = math.tan(math.pi * 1681.974450955533 / fs)
    Q = 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    K = math.tan(math.pi * 38.13547087602444 / fs)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    high = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.asarray(shelf + high, dtype=np.float64)


def check_rate(sampling_rate) -> int:
    fs = A.as_int(sampling_rate, "sampling_rate")
    if not MIN_RATE <= fs <= MAX_RATE or fs % 10:
        raise ValueError(f"sampling_rate must lie in {MIN_RATE} .. {MAX_RATE} Hz and be a multiple of 10 (100 ms blocks), got {sampling_rate!r}")
    return fs


class _Loudness(torch.nn.Module):
    """what the meter and the normaliser share: the checks, the coefficients, the workspace and the call"""

    def __init__(self, device, sampling_rate: int, target_lufs: float, peak_ceiling: Optional[float], max_wav_value: float):
        super().__init__()
        self.dev = None if device is None else torch.device(device)
        self.sampling_rate = check_rate(sampling_rate)
        self.target_lufs = float(target_lufs)
        if not math.isfinite(self.target_lufs):
            raise ValueError(f"target_lufs must be finite, got {target_lufs!r}")
        if peak_ceiling is not None and not (float(peak_ceiling) > 0.0 and math.isfinite(float(peak_ceiling))):
            raise ValueError(f"peak_ceiling must be None or a positive number, got {peak_ceiling!r}")
        self.peak_ceiling = None if peak_ceiling is None else float(peak_ceiling)
        self.max_wav_value = A.max_wav(max_wav_value)
        self.coefficients = k_weighting(self.sampling_rate)
        self._kw = (ctypes.c_double * 10)(*self.coefficients.tolist())
        self._ws = A.Cache(capacity=5)   # (device, B, n) -> workspace

    def _run(self, who: str, audio: torch.Tensor, lengths: Optional[torch.Tensor], scale_out: bool):
        audio = A.signal(audio, "audio", who)
        B, n = audio.shape
        lib = L_.load()
        L_.require_device()
        dev = audio.device
        li = A.device_lengths(lengths, B, n, dev)
        out = torch.empty(B, n, dtype=torch.float32, device=dev) if scale_out else None
        lufs = torch.empty(B, dtype=torch.float64, device=dev)
        gains = torch.empty(B, dtype=torch.float32, device=dev)
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        blocks = torch.empty(B, 2, dtype=torch.int32, device=dev)
        ws = self._ws.get((dev, B, n),
                          lambda: torch.empty(int(lib.efts_loudness_workspace_bytes(B, n, self.sampling_rate)), dtype=torch.uint8, device=dev))
        ceiling = self.peak_ceiling if self.peak_ceiling is not None else 0.0
        fn, name, scale = A.pcm_entry(lib, "efts_loudness", audio, self.max_wav_value)
        with O.stream_scope():
            L_.check(fn(audio.data_ptr(), n, li.data_ptr(), self.sampling_rate, self._kw, self.target_lufs, ceiling, *scale,
                        None if out is None else out.data_ptr(), n, lufs.data_ptr(), gains.data_ptr(), flags.data_ptr(), blocks.data_ptr(),
                        ws.data_ptr(), B, O._stream()), name)
        return out, lufs, gains, flags, blocks


class LoudnessMeter(_Loudness):
    """lufs = LoudnessMeter(device, sampling_rate)(audio [B, n] float32 | int16, lengths=None)

    lufs: float64 [B], the integrated loudness of every item in LUFS; -inf for an item without a block over the absolute gate (silence, or
    shorter than 0.4 s).  int16 PCM is taken as x / max_wav_value.  Every item is treated exactly as if it had been passed alone."""

    def __init__(self, device=None, sampling_rate: int = 22050, max_wav_value: float = 32768.0):
        super().__init__(device, sampling_rate, -23.0, None, max_wav_value)

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._run("LoudnessMeter", audio, lengths, scale_out=False)[1]


class LoudnessNormalizer(_Loudness):
    """out = LoudnessNormalizer(device, sampling_rate, target_lufs, peak_ceiling)(audio [B, n] float32 | int16, lengths=None)

    out: fp32 [B, n], every item multiplied by the one gain that brings its integrated loudness to `target_lufs`, zero behind its length.
    With `peak_ceiling` a gain that would take the item's peak above it is cut back so that no sample exceeds it (flag bit 1); None
    switches that off.  An item without a loudness (flag bit 0) keeps its level.  With `return_stats=True` also lufs float64 [B] (measured,
    before the gain), gains fp32 [B] (what every sample was multiplied by, 1 / max_wav_value included for int16), flags int32 [B] and
    blocks int32 [B, 2] (400 ms blocks over the absolute gate, and over both gates).  Lengths do not change."""

    def __init__(self, device=None, sampling_rate: int = 22050, target_lufs: float = -23.0, peak_ceiling: Optional[float] = 0.99,
                 max_wav_value: float = 32768.0):
        super().__init__(device, sampling_rate, target_lufs, peak_ceiling, max_wav_value)

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None, return_stats: bool = False):
        out, lufs, gains, flags, blocks = self._run("LoudnessNormalizer", audio, lengths, scale_out=True)
        if return_stats:
            return out, lufs, gains, flags, blocks
        return out
