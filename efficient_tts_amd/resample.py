"""On-device sample-rate conversion between integer rates: corpora recorded at another rate than the front-end's, output at another
rate than the vocoder's.

The filter is a band-limited windowed-sinc interpolator (Kaiser window) between `src` and `dst`:

    g = gcd(src, dst), L = dst / g, M = src / g;  fc = rolloff * min(1, dst / src);  W = ceil(Z / fc), K = 2 W + 1
    h(tau) = fc sinc(u) I0(beta sqrt(1 - (u / Z)^2)) / I0(beta), u = fc tau, for |u| < Z and 0 otherwise  (tau in source samples)
    y[n] = sum over k = -W .. W of x[i0 + k] h(p / L - k),  i0 = floor(n M / L), p = (n M) mod L,  x = 0 outside [0, len)
    out_len = (len L + M - 1) // M

`quality="best"`: Z 64, beta 14.77, rolloff 0.9476; `"fast"`: Z 16, beta 8.555, rolloff 0.85.  The polyphase table h[p][k + W], [L, K],
is computed once per (src, dst, quality) on the host in float64 and kept as fp32 in device memory (as `GriffinLimVocoder` keeps its
pseudo-inverse); the sums run in csrc/efts_resample.hip (`efts_resample`, `efts_resample_pcm16`): fp32, one fixed order, no atomics.
No CPU path: the HIP library is required.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import audio_args as A
from . import lib as L_
from . import ops as O

QUALITIES = {"best": dict(Z=64, beta=14.77, rolloff=0.9476), "fast": dict(Z=16, beta=8.555, rolloff=0.85)}
TABLE_MAX_BYTES = 4 << 20


def _rate(value, name: str) -> int:
    if A.as_int(value, name) <= 0:
        raise ValueError(f"{name} must be a positive integer (Hz), got {value!r}")
    return int(value)


def _geometry(src, dst, quality: str) -> Tuple[int, int, int, float, dict]:
    src, dst = _rate(src, "src"), _rate(dst, "dst")
    if quality not in QUALITIES:
        raise ValueError(f"quality must be one of {sorted(QUALITIES)}, got {quality!r}")
    q = QUALITIES[quality]
    g = math.gcd(src, dst)
    L, M = dst // g, src // g
    fc = q["rolloff"] * min(1.0, dst / src)
    W = int(math.ceil(q["Z"] / fc))
    if L * (2 * W + 1) * 4 > TABLE_MAX_BYTES:
        raise ValueError(f"{src} -> {dst} Hz needs a table of {L} x {2 * W + 1} floats, more than {TABLE_MAX_BYTES >> 20} MiB: choose rates with a larger common divisor")
    return L, M, W, fc, q


def resample_length(n: int, src: int, dst: int) -> int:
    """samples that `n` samples at `src` Hz become at `dst` Hz"""
    src, dst = _rate(src, "src"), _rate(dst, "dst")
    g = math.gcd(src, dst)
    L, M = dst // g, src // g
    return (int(n) * L + M - 1) // M


def resample_table(src: int, dst: int, quality: str = "best") -> Tuple[torch.Tensor, int, int, int]:
    """(table fp32 [L, K], L, M, W): table[p][k + W] = h(p / L - k), float64 on the host, rounded once to fp32"""
    L, M, W, fc, q = _geometry(src, dst, quality)
    tau = np.arange(L, dtype=np.float64)[:, None] / L - np.arange(-W, W + 1, dtype=np.float64)[None, :]
    u = fc * tau
    inside = np.abs(u) < q["Z"]
    window = np.i0(q["beta"] * np.sqrt(np.clip(1.0 - (u / q["Z"]) ** 2, 0.0, None))) / np.i0(q["beta"])
    h = np.where(inside, fc * np.sinc(u) * window, 0.0)
    return torch.from_numpy(h.astype(np.float32)).contiguous(), L, M, W


class Resampler(torch.nn.Module):
    """out, out_lengths = Resampler(device, src_rate, dst_rate)(audio [B, n] float32 | int16, lengths=None)

    out: fp32 [B, resample_length(n)], zero past each item's converted length; out_lengths: int64 [B].  int16 PCM is scaled by
    1 / max_wav_value at the kernel's loads (what `LogMelFrontend` does with it).  Every item is converted exactly as if it had been
    passed alone.  `src_rate == dst_rate` is the identity: no launch, the samples are returned as fp32 (int16 scaled as above)."""

    def __init__(self, device=None, src_rate: int = 22050, dst_rate: int = 22050, quality: str = "best", max_wav_value: float = 32768.0):
        super().__init__()
        self.dev = None if device is None else torch.device(device)
        self.src_rate, self.dst_rate, self.quality = _rate(src_rate, "src_rate"), _rate(dst_rate, "dst_rate"), quality
        self.max_wav_value = float(max_wav_value)
        self.identity = self.src_rate == self.dst_rate
        if self.identity:
            _geometry(self.src_rate, self.dst_rate, quality)          # (the quality is still checked)
            self._table_host, self.L, self.M, self.W = None, 1, 1, 0
        else:
            self._table_host, self.L, self.M, self.W = resample_table(self.src_rate, self.dst_rate, quality)
        self._tables = {}                # device -> table

    def out_length(self, n: int) -> int:
        return (int(n) * self.L + self.M - 1) // self.M

    def lengths_of(self, lengths: torch.Tensor) -> torch.Tensor:
        return torch.div(lengths.to(torch.int64) * self.L + (self.M - 1), self.M, rounding_mode="floor")

    def _table(self, dev) -> torch.Tensor:
        if dev not in self._tables:
            self._tables[dev] = self._table_host.to(dev)
        return self._tables[dev]

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        audio = A.signal(audio, "audio", None if self.identity else "Resampler")         # (the identity has no launch and takes host tensors too)
        B, n = audio.shape
        dev = audio.device
        li = A.device_lengths(lengths, B, n, dev)
        if self.identity:
            return (audio if audio.dtype == torch.float32 else audio.to(torch.float32) * (1.0 / self.max_wav_value)), li.to(torch.int64)
        lib = L_.load()
        L_.require_device()
        n_out = self.out_length(n)
        out = torch.empty(B, n_out, dtype=torch.float32, device=dev)
        out_lens = torch.empty(B, dtype=torch.int32, device=dev)
        table = self._table(dev)
        fn, name, scale = A.pcm_entry(lib, "efts_resample", audio, self.max_wav_value)
        with O.stream_scope():
            L_.check(fn(audio.data_ptr(), n, *scale, li.data_ptr(), table.data_ptr(), self.L, self.M, self.W, out.data_ptr(), n_out,
                        out_lens.data_ptr(), B, O._stream()), name)
        return out, out_lens.to(torch.int64)
