"""On-device mel-cepstra of waveforms and the mel-cepstral distortion (MCD) that TTS and vocoder papers report for spectral quality: an
order-24 all-pass-warped mel-cepstrum per frame, compared along a dynamic-time-warping path (synthesis against a recording) or frame by
frame (copy-synthesis, which is time-aligned).

    frames   those of `stft.STFTMagnitude` at n_fft = 1024: periodic Hann window of win_length, centred, reflect padding, T = 1 + L // hop
    L[f]     ln max(re^2 + im^2, 1e-7), f = 0 .. K = n_fft / 2: the log periodogram
    c^       the one-sided cepstrum of ln|X| = L / 2:  ln|X(w_f)| = sum_{n = 0 .. K} c^[n] cos(n w_f)
    mc       the frequency transform of c^ to the all-pass-warped axis w~ = w + 2 atan2(alpha sin w, 1 - alpha cos w), truncated to
             c~[1 .. order] (Oppenheim's recursion, as SPTK's `freqt`); c~[0], the level, is left out
    mcd      (10 / ln 10) sqrt(2) (sum of ||mc_a[i] - mc_b[j]||_2 over the paired frames) / (number of pairs)   dB

Every step from L to mc is linear, so the whole analysis is ONE table [order, K + 1] (`mcep_table`, float64 on the host, rounded once to
fp32) applied to L, and the hot path is one launch (`efts_logspec_project`, csrc/efts_mcep.hip): frame, window, FFT, ln and the projection,
with no spectrogram in memory.  include/efts_abi.h has the definition, summation order included; tests/mcep_reference.py restates it in
numpy float64.  No CPU path: the HIP library is required.

What this is: the periodogram route -- the frequency transform of the FFT cepstrum, which is what SPTK's conversion of a spectrum to a
mel-cepstrum does.  What it is not: the iterative `mcep` analysis (unbiased estimation of the log spectrum), and not a WORLD / STRAIGHT
envelope; absolute values sit near, not on, numbers from those pipelines.  There is no per-frame silence gating: every frame counts
(`bin/score.py --trim_silence` cuts the ends of the recordings, nothing more).  `pysptk` was not available to compare against.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import audio_args as A
from . import lib as L_
from . import ops as O
from . import score as S
from .stft import hann_window

N_FFT, MAX_ORDER = 1024, 32                      # limits of efts_logspec_project (include/efts_abi.h)
ALPHAS = {16000: 0.42, 22050: 0.455, 24000: 0.466, 44100: 0.544, 48000: 0.554}      # the all-pass constant that approximates the mel scale


def default_alpha(sampling_rate: int) -> float:
    if sampling_rate not in ALPHAS:
        raise ValueError(f"no default alpha for {sampling_rate} Hz (known: {sorted(ALPHAS)}): pass alpha explicitly")
    return ALPHAS[sampling_rate]


def freqt_matrix(n_in: int, order: int, alpha: float) -> np.ndarray:
    """A(alpha), float64 [order + 1, n_in]: column n is the frequency transform of the unit cepstrum e_n, truncated to c~[0 .. order]"""
    g = np.zeros((order + 1, n_in), dtype=np.float64)
    beta = 1.0 - alpha * alpha
    for i in range(n_in - 1, -1, -1):
        d = g.copy()
        g[0] = alpha * d[0]
        g[0, i] += 1.0
        if order >= 1:
            g[1] = beta * d[0] + alpha * d[1]
        for j in range(2, order + 1):
            g[j] = d[j - 1] + alpha * (d[j] - g[j - 1])
    return g


def mcep_table(n_fft: int = N_FFT, order: int = 24, alpha: float = 0.455) -> np.ndarray:
    """float64 [order, n_fft / 2 + 1]: rows 1 .. order of 1/2 A(alpha) diag(w) D, the map from ln(power spectrum) to c~[1 .. order]"""
    n_fft, order = A.as_int(n_fft, "n_fft"), A.as_int(order, "order")
    if n_fft < 4 or n_fft & (n_fft - 1):
        raise ValueError(f"n_fft must be a power of two >= 4, got {n_fft}")
    K = n_fft // 2
    if not 1 <= order <= min(MAX_ORDER, K):
        raise ValueError(f"order must lie in 1 .. {min(MAX_ORDER, K)}, got {order}")
    alpha = float(alpha)
    if not -1.0 < alpha < 1.0:
        raise ValueError(f"alpha must lie in (-1, 1), got {alpha!r}")
    n = np.arange(K + 1, dtype=np.float64)
    s = np.where((n == 0) | (n == K), 1.0, 2.0)
    w = np.where((n == 0) | (n == K), 0.5, 1.0)
    D = s[None, :] * np.cos(np.pi * n[:, None] * n[None, :] / K) / K
    return 0.5 * (freqt_matrix(K + 1, order, alpha)[1:] @ (w[:, None] * D))


class MelCepstrum(torch.nn.Module):
    """mc, frames = MelCepstrum(device, sampling_rate=22050, n_fft=1024, hop_size=256, win_length=1024, order=24, alpha=None)(audio, lengths=None)

    audio [B, n] float32 or int16 (scaled by 1 / max_wav_value).  mc: fp32 [B, 1 + n // hop_size, order], c~[1 .. order] per frame, zero at
    and beyond an item's frame count; frames: int32 [B] on the device (0 for an item of at most n_fft / 2 samples).  `alpha` defaults by
    rate (0.42 at 16 kHz, 0.455 at 22.05 kHz, 0.466 at 24 kHz, 0.544 at 44.1 kHz, 0.554 at 48 kHz).  One launch, nothing read back."""

    def __init__(self, device=None, sampling_rate: int = 22050, n_fft: int = N_FFT, hop_size: int = 256, win_length: int = 1024, order: int = 24,
                 alpha: Optional[float] = None, max_wav_value: float = 32768.0):
        super().__init__()
        self.dev = None if device is None else torch.device(device)
        self.sampling_rate = A.as_int(sampling_rate, "sampling_rate")
        if self.sampling_rate < 1:
            raise ValueError("sampling_rate must be positive")
        self.n_fft, self.hop, self.win_length = A.as_int(n_fft, "n_fft"), A.as_int(hop_size, "hop_size"), A.as_int(win_length, "win_length")
        if self.n_fft != N_FFT:
            raise ValueError(f"n_fft must be {N_FFT}, got {n_fft!r}")
        if not 1 <= self.hop <= self.n_fft:
            raise ValueError(f"hop_size must lie in 1 .. n_fft, got {hop_size!r}")
        if not 2 <= self.win_length <= self.n_fft:
            raise ValueError(f"win_length must lie in 2 .. n_fft, got {win_length!r}")
        self.alpha = default_alpha(self.sampling_rate) if alpha is None else float(alpha)
        self.table = mcep_table(self.n_fft, order, self.alpha).astype(np.float32)           # (checks order and alpha)
        self.order = self.table.shape[0]
        self.max_wav_value = A.max_wav(max_wav_value)
        self._consts = {}                # device -> (window, table)

    def _on(self, dev):
        if dev not in self._consts:
            self._consts[dev] = (torch.from_numpy(hann_window(self.win_length)).to(dev), torch.from_numpy(self.table).to(dev).contiguous())
        return self._consts[dev]

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        audio = A.signal(audio, "audio", "efficient_tts_amd.mcep")
        B, n = audio.shape
        lib = L_.load()
        L_.require_device()
        dev = audio.device
        li = A.device_lengths(lengths, B, n, dev)
        window, table = self._on(dev)
        mc = torch.empty(B, 1 + n // self.hop, self.order, dtype=torch.float32, device=dev)
        frames = torch.empty(B, dtype=torch.int32, device=dev)
        with O.stream_scope():
            L_.check(lib.efts_logspec_project(audio.data_ptr(), int(audio.dtype == torch.int16), 1.0 / self.max_wav_value, n, li.data_ptr(), n,
                                              window.data_ptr(), table.data_ptr(), self.order, mc.data_ptr(), frames.data_ptr(), B, self.n_fft, self.hop,
                                              self.win_length, O._stream()), "efts_logspec_project")
        return mc, frames


@torch.no_grad()
def frame_dist(x: torch.Tensor, x_frames: torch.Tensor, y: torch.Tensor, y_frames: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(cost [B] float64, count [B] int32): frames t = 0 .. min(x_frames[b], y_frames[b]) - 1 of x [B, Tx, D] and y [B, Ty, D] paired one to
    one, cost the sum of ||x[t] - y[t]||_2 in frame order -- `score.dtw`'s local cost --, count the number of pairs; (NaN, 0) without one"""
    x, xl = S._rows("x", x, x_frames)
    y, yl = S._rows("y", y, y_frames)
    if y.shape[0] != x.shape[0] or y.shape[2] != x.shape[2] or y.device != x.device:
        raise ValueError("x and y must agree in B, D and device")
    B, Tx, D = x.shape
    lib = L_.load()
    L_.require_device()
    cost = torch.empty(B, dtype=torch.float64, device=x.device)
    count = torch.empty(B, dtype=torch.int32, device=x.device)
    with O.stream_scope():
        L_.check(lib.efts_frame_dist(x.data_ptr(), x.stride(1), x.stride(0), xl.data_ptr(), Tx, y.data_ptr(), y.stride(1), y.stride(0), yl.data_ptr(),
                                     y.shape[1], D, cost.data_ptr(), count.data_ptr(), B, O._stream()), "efts_frame_dist")
    return cost, count


class WaveformMCD(torch.nn.Module):
    """out = WaveformMCD(device, <the arguments of MelCepstrum>)(a [B, n], len_a, b [B, m], len_b, *, aligned=False, return_path=False)

    Mel-cepstral distortion between two waveform batches, per item, as a dict of device tensors: `mcd` [B] in dB, `cost` and `count` [B]
    (the summed distance and the number of frame pairs behind it), `frames_a` / `frames_b` [B] int32.  Warped (the default): the pairs
    are the cells of the cheapest DTW path (`score.dtw` on the two cepstra, unchanged: cost fp32, count the path length; at most 8192
    frames per side); `return_path=True` runs `score.dtw_path` instead and adds `path`.  `aligned=True`: frames t = 0 .. min(Ta, Tb) - 1 are
    paired one to one (cost float64) -- for copy-synthesis, where both signals share one time axis.  An item without a frame on either
    side has mcd NaN and count 0.  Three launches; no host synchronisation."""

    def __init__(self, device=None, **kwargs):
        super().__init__()
        self.cepstrum = MelCepstrum(device, **kwargs)

    @torch.no_grad()
    def forward(self, a: torch.Tensor, len_a: Optional[torch.Tensor], b: torch.Tensor, len_b: Optional[torch.Tensor], *, aligned: bool = False,
                return_path: bool = False) -> Dict[str, torch.Tensor]:
        if aligned and return_path:
            raise ValueError("aligned=True pairs the frames one to one: there is no path to return")
        mc_a, fa = self.cepstrum(a, len_a)
        mc_b, fb = self.cepstrum(b, len_b)
        extra = {}
        if aligned:
            cost, count = frame_dist(mc_a, fa, mc_b, fb)
        elif return_path:
            cost, count, extra["path"] = S.dtw_path(mc_a, fa, mc_b, fb)
        else:
            cost, count = S.dtw(mc_a, fa, mc_b, fb)
        return dict(mcd=S.MCD_DB * cost / count, cost=cost, count=count, frames_a=fa, frames_b=fb, **extra)
