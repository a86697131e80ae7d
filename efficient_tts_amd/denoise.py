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

For corpora the same chain runs as a spectral gate with a noise profile per recording: `NoiseProfile` measures the mean magnitude spectrum
of an item's own quiet frames (`efts_noise_profile`), `SpectralGate` subtracts `strength` times it with a floor under the gain
(`efts_spectral_gate`, the same kernel body) and leaves an item without enough quiet frames as it came.
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


def check_floor(value) -> float:
    f = float(value)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"floor must lie in 0 .. 1, got {value!r}")
    return f


def check_top_db(value) -> float:
    t = float(value)
    if not (t > 0.0 and math.isfinite(t)):
        raise ValueError(f"top_db must be a finite number > 0, got {value!r}")
    return t


def check_min_frames(value) -> int:
    k = A.as_int(value, "min_frames")
    if k < 1:
        raise ValueError(f"min_frames must be >= 1, got {value!r}")
    return k


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
        if audio.numel() <= N_FFT // 2:        # (a generator of few samples per frame: HiFi-GAN V1 and C8C8I make 256, 88 frames are 22528 samples)
            raise ValueError(f"BiasDenoiser.from_vocoder: {audio.numel()} samples from {frames} frames hold no {N_FFT}-point STFT frame; raise `frames`")
        with torch.no_grad():
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


class _Windowed(torch.nn.Module):
    """what the two corpus modules below share: the window per device and the arguments of a padded batch"""

    def __init__(self, device=None):
        super().__init__()
        self.dev = None if device is None else torch.device(device)
        self._windows = {}

    def _window(self, dev):
        if dev not in self._windows:
            self._windows[dev] = torch.from_numpy(hann_window(N_FFT)).to(dev)
        return self._windows[dev]

    def _batch(self, audio, lengths, who):
        audio = A.signal(audio, "audio", who)
        B, n = audio.shape
        lib = L_.load()
        L_.require_device()
        return audio, B, n, lib, A.device_lengths(lengths, B, n, audio.device)


class NoiseProfile(_Windowed):
    """stats = NoiseProfile(device, top_db=40.0, min_frames=8, max_wav_value=32768.0)(audio [B, L] float32 or int16, lengths=None)

    The stationary floor of every item, measured from its own quiet frames: with e[t] the energy of the windowed frame t (N = 1024, hop 256,
    the framing of `BiasDenoiser`), the frames with e[t] * 10^(top_db / 10) < max e -- the rule of `SilenceTrimmer`, no logarithm -- are the
    noise frames, and the profile is the mean of their magnitude spectra.  stats: a dict of device tensors, nothing is read back:
    `profile` fp32 [B, 513] (exactly 0 for an item with fewer than `min_frames` noise frames), `noise_frames` and `frames` int32 [B], `noise_db`
    float64 [B] (the noise frames' mean energy under the loudest frame's; NaN without a noise frame).  `efts_noise_profile`, four launches."""

    def __init__(self, device=None, top_db: float = 40.0, min_frames: int = 8, max_wav_value: float = 32768.0):
        super().__init__(device)
        self.top_db, self.min_frames, self.max_wav_value = check_top_db(top_db), check_min_frames(min_frames), A.max_wav(max_wav_value)
        self.ratio = float(10.0 ** (np.float64(self.top_db) / 10.0))        # r, float64, once
        self._ws = A.Cache(capacity=5)   # (device, B, n) -> workspace

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        audio, B, n, lib, li = self._batch(audio, lengths, "NoiseProfile")
        dev = audio.device
        pcm = audio.dtype == torch.int16
        profile = torch.empty(B, BINS, dtype=torch.float32, device=dev)
        counts = torch.empty(2, B, dtype=torch.int32, device=dev)
        noise_db = torch.empty(B, dtype=torch.float64, device=dev)
        nbytes = int(lib.efts_noise_profile_workspace_bytes(B, n))
        ws = self._ws.get((dev, B, n), lambda: torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev))
        with O.stream_scope():
            L_.check(lib.efts_noise_profile(audio.data_ptr(), int(pcm), 1.0 / self.max_wav_value if pcm else 1.0, n, li.data_ptr(), n,
                                            self._window(dev).data_ptr(), self.ratio, self.min_frames, profile.data_ptr(), BINS, counts[0].data_ptr(),
                                            counts[1].data_ptr(), noise_db.data_ptr(), ws.data_ptr(), nbytes, B, O._stream()), "efts_noise_profile")
        return {"profile": profile, "noise_frames": counts[0], "frames": counts[1], "noise_db": noise_db}


class SpectralGate(_Windowed):
    """out = SpectralGate(device, strength=1.0, floor=0.1, top_db=40.0, min_frames=8)(audio [B, L] float32 or int16, lengths=None, profile=None,
                                                                                    strength=None, floor=None, return_stats=False)

    Spectral subtraction with a gain floor: per frame and bin g = max((m - strength * profile) / m, floor) (0 below the profile before the
    floor), at the frame's own phase, through the STFT / inverse STFT / overlap-add of `BiasDenoiser` in one launch (`efts_spectral_gate`).
    Without `profile` every item is gated with the profile that `NoiseProfile` measures from its own quiet frames; an item with fewer than
    `min_frames` of them is returned as it came (the flags are built on the device, nothing is read back).  With `profile`, [513] for the
    batch or [B, 513] per item -- a room-tone recording's, for instance --, nothing is bypassed.  out: fp32 [B, L], zero behind an item's
    length; int16 PCM comes back as sample / max_wav_value.  With `return_stats=True` also the dict of `NoiseProfile` (None with a given
    profile).  `strength` and `floor` override the module's for one call and are passed by value."""

    def __init__(self, device=None, strength: float = 1.0, floor: float = 0.1, top_db: float = 40.0, min_frames: int = 8, max_wav_value: float = 32768.0):
        super().__init__(device)
        self.strength, self.floor = check_strength(strength), check_floor(floor)
        self.measure = NoiseProfile(device, top_db=top_db, min_frames=min_frames, max_wav_value=max_wav_value)
        self.top_db, self.min_frames, self.max_wav_value = self.measure.top_db, self.measure.min_frames, self.measure.max_wav_value

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None, profile: Optional[torch.Tensor] = None,
                strength: Optional[float] = None, floor: Optional[float] = None, return_stats: bool = False):
        s = self.strength if strength is None else check_strength(strength)
        fl = self.floor if floor is None else check_floor(floor)
        if profile is not None and tuple(profile.shape) not in ((BINS,), (audio.shape[0], BINS)):
            raise ValueError(f"profile must be [{BINS}] or [B, {BINS}], got {tuple(profile.shape)}")
        audio, B, n, lib, li = self._batch(audio, lengths, "SpectralGate")
        dev = audio.device
        pcm = audio.dtype == torch.int16
        stats = bypass = None
        if profile is None:
            stats = self.measure(audio, li)
            profile, ld_profile = stats["profile"], BINS
            bypass = (stats["noise_frames"] < self.min_frames).to(torch.int32)
        else:
            profile = profile.to(device=dev, dtype=torch.float32).contiguous()
            ld_profile = 0 if profile.dim() == 1 else BINS
        out = torch.empty(B, n, dtype=torch.float32, device=dev)
        frames = torch.empty(B, dtype=torch.int32, device=dev)
        with O.stream_scope():
            L_.check(lib.efts_spectral_gate(audio.data_ptr(), int(pcm), 1.0 / self.max_wav_value if pcm else 1.0, n, li.data_ptr(), n,
                                            self._window(dev).data_ptr(), profile.data_ptr(), ld_profile, s, fl,
                                            None if bypass is None else bypass.data_ptr(), out.data_ptr(), n, frames.data_ptr(), B, O._stream()),
                     "efts_spectral_gate")
        return (out, stats) if return_stats else out
