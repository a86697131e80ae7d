"""On-device spectral denoiser for a vocoder's bias noise: a HiFi-GAN generator fed a constant mel does not answer with silence but with a
faint stationary tone-and-hiss pattern, which sits under every utterance.  The remedy of the published Tacotron 2 / WaveGlow / HiFi-GAN
inference scripts: measure that pattern's magnitude spectrum once, then subtract `strength` times it from every frame's magnitudes.

With N = 1024, hop 256, w the periodic Hann window (float64 on the host, rounded once), per item of len samples:

    frames   T = 1 + len // 256, centred, 512 samples of reflect padding at both ends (those of `stft.STFTMagnitude`); len <= 512: no frames
    X = DFT(w * frame);  m = |X|;  d = m - strength * bias[f];  g = d / m if d > 0 else 0;  x' = real inverse DFT of g X
    out[s] = (sum over the frames covering s, oldest first, of w * x') / max(sum of their w^2, 1e-8) for s < len, 0 behind

which is torch.stft(center=True, pad_mode="reflect") -> gain -> torch.istft(center=True, length=len).  An item of at most 512 samples is
passed through bit for bit.  include/efts_abi.h has the full definition, the order of every sum included.  It runs in csrc/efts_denoise.hip
(`efts_denoise`) as ONE launch: no spectrum and no frame goes to memory, no atomics, nothing read back by the host.  No CPU path: the HIP
library is required.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import audio_args as A
from . import lib as L_
from . import ops as O
from .stft import STFTMagnitude, hann_window

N_FFT, HOP, BINS = 1024, 256, 513


def check_strength(value) -> float:
    s = float(value)
    if not (s >= 0.0 and math.isfinite(s)):
        raise ValueError(f"strength must be a finite number >= 0, got {value!r}")
    return s


class BiasDenoiser(torch.nn.Module):
    """out = BiasDenoiser(device, bias, strength=0.01)(audio [B, L] float32, lengths=None, strength=None, return_frames=False)

    bias: [513] non-negative magnitudes (tensor or array), what `STFTMagnitude(device, 1024, 256, 1024)` gives for the vocoder's answer to
    a blank mel (`from_vocoder` measures it).  out: fp32 [B, L], zero behind an item's length; with `return_frames=True` also frames int32
    [B] (0 for an item of at most 512 samples, which is returned as it came).  `strength` overrides the module's for one call; it is passed
    by value, so a sweep needs no new graph capture.  Every item is treated exactly as if it had been passed alone."""

    def __init__(self, device=None, bias=None, strength: float = 0.01):
        super().__init__()
        self.dev = None if device is None else torch.device(device)
        if bias is None:
            raise ValueError("bias [513] is required (BiasDenoiser.from_vocoder measures it)")
        b = torch.as_tensor(np.asarray(bias.detach().cpu()) if isinstance(bias, torch.Tensor) else np.asarray(bias)).to(torch.float32)
        if b.shape != (BINS,):
            raise ValueError(f"bias must be [{BINS}], got {tuple(b.shape)}")
        if not bool(torch.isfinite(b).all()) or bool((b < 0).any()):
            raise ValueError("bias must hold finite, non-negative magnitudes")
        self.strength = check_strength(strength)
        self.bias = b.contiguous()
        self._dev_args = {}              # device -> (window, bias)
        self._ws = A.Cache(capacity=5)   # (device, B, n) -> workspace (the present kernel asks for none)

    def _args(self, dev):
        if dev not in self._dev_args:
            self._dev_args[dev] = (torch.from_numpy(hann_window(N_FFT)).to(dev), self.bias.to(dev))
        return self._dev_args[dev]

    @classmethod
    def from_vocoder(cls, vocoder, device, frames: int = 88, mel_value: float = 0.0, num_mels: int = 80, strength: float = 0.01):
        """the published recipe: `vocoder(mel)` once on a [1, num_mels, frames] mel filled with `mel_value` (math.log(1e-5) is the front-end's
        silence), the 1024 / 256 / 1024 STFT magnitudes of the answer, frame 0 as the bias.  Any callable with the vocoders' signature."""
        device = torch.device(device)
        mel = torch.full((1, A.as_int(num_mels, "num_mels"), A.as_int(frames, "frames")), float(mel_value), dtype=torch.float32, device=device)
        with torch.no_grad():
            audio = vocoder(mel)
            mag, _ = STFTMagnitude(device, N_FFT, HOP, N_FFT)(audio.reshape(1, -1).float())
        return cls(device, mag[0, 0], strength=strength)

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None, strength: Optional[float] = None, return_frames: bool = False):
        if audio.dtype == torch.int16:
            raise ValueError("BiasDenoiser takes float32 samples (int16 PCM is not supported: convert it first)")
        s = self.strength if strength is None else check_strength(strength)
        audio = A.signal(audio, "audio", "BiasDenoiser")
        B, n = audio.shape
        lib = L_.load()
        L_.require_device()
        dev = audio.device
        li = A.device_lengths(lengths, B, n, dev)
        window, bias = self._args(dev)
        out = torch.empty(B, n, dtype=torch.float32, device=dev)
        frames = torch.empty(B, dtype=torch.int32, device=dev)
        nbytes = int(lib.efts_denoise_workspace_bytes(B, n))
        ws = self._ws.get((dev, B, n), lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev)) if nbytes else None
        with O.stream_scope():
            L_.check(lib.efts_denoise(audio.data_ptr(), n, li.data_ptr(), n, window.data_ptr(), bias.data_ptr(), s, out.data_ptr(), n,
                                      frames.data_ptr(), None if ws is None else ws.data_ptr(), nbytes, B, O._stream()), "efts_denoise")
        return (out, frames) if return_frames else out
