"""On-device silence trimming and peak normalisation of a padded batch of recordings: what `librosa.effects.trim` and
`normalize(audio) * 0.95` do offline, as one step of the device-side data path (behind `Resampler`, in front of `LogMelFrontend`).

With frame length W, hop H, pad = (W - H) / 2, r = 10^(top_db / 10) and x = 0 outside an item's [0, len):

    T = ceil(len / H);  E_t = sum of x^2 over samples t H - pad .. t H - pad + W - 1;  E_max = max_t E_t
    frame t is sound iff (double) E_t * r > (double) E_max            (E_max == 0: no frame is sound)
    start = max(0, (t_first - keep_frames) H),  end = min(len, (t_last + 1 + keep_frames) H);  no sound frame: 0 .. len, gain 1
    p = max |x| over [start, end);  gain = peak / p (one fp32 division) when `peak` is given and p > 0, else 1 (int16: 1 / max_wav_value)
    out[i] = x[start + i] * gain for i < end - start, 0 behind

int16 energies are exact integers, so the decision is reproducible to the bit; include/efts_abi.h has the full definition, fp32 summation
order included.  The sums run in csrc/efts_trim.hip (`efts_trim`, `efts_trim_pcm16`): three launches, no atomics, nothing read back by the
host.  No CPU path: the HIP library is required.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import audio_args as A
from . import lib as L_
from . import ops as O

FRAME_LENGTHS = (512, 1024, 2048)


class SilenceTrimmer(torch.nn.Module):
    """out, out_lengths = SilenceTrimmer(device, frame_length, hop_size, top_db, keep_frames, peak)(audio [B, n] float32 | int16, lengths=None)

    out: fp32 [B, n], every item moved to the front of its row and zero behind its new length; out_lengths: int64 [B].  With
    `return_bounds=True` also starts int64 [B] (the first sample kept) and gains fp32 [B] (what every kept sample was multiplied by).
    `peak=None` leaves the level alone (int16 PCM is scaled by 1 / max_wav_value, what `LogMelFrontend` does with it at its loads);
    `trim=False` leaves the bounds alone (0 .. len for every item): normalisation only.  Every item is treated exactly as if it had been
    passed alone."""

    def __init__(self, device=None, frame_length: int = 1024, hop_size: int = 256, top_db: float = 40.0, keep_frames: int = 2,
                 peak: Optional[float] = None, max_wav_value: float = 32768.0, trim: bool = True):
        super().__init__()
        self.dev = None if device is None else torch.device(device)
        self.frame_length, self.hop = A.as_int(frame_length, "frame_length"), A.as_int(hop_size, "hop_size")
        if self.frame_length not in FRAME_LENGTHS:
            raise ValueError(f"frame_length must be one of {FRAME_LENGTHS}, got {frame_length!r}")
        if not 1 <= self.hop <= self.frame_length or (self.frame_length - self.hop) % 2:
            raise ValueError(f"hop_size must lie in 1 .. frame_length with frame_length - hop_size even, got {hop_size!r}")
        self.top_db = float(top_db)
        if not self.top_db > 0.0 or not np.isfinite(self.top_db):
            raise ValueError(f"top_db must be > 0, got {top_db!r}")
        self.keep_frames = A.as_int(keep_frames, "keep_frames")
        if self.keep_frames < 0:
            raise ValueError(f"keep_frames must be >= 0, got {keep_frames!r}")
        if peak is not None and not 0.0 < float(peak) <= 1.0:
            raise ValueError(f"peak must be None or lie in (0, 1], got {peak!r}")
        self.peak = None if peak is None else float(peak)
        self.max_wav_value = A.max_wav(max_wav_value)
        self.trim = bool(trim)
        self.ratio = float(10.0 ** (np.float64(self.top_db) / 10.0))        # r, float64, once
        if not self.ratio > 1.0 or not np.isfinite(self.ratio):
            raise ValueError(f"top_db {top_db!r} gives no usable threshold ratio")
        self._ws = A.Cache(capacity=5)   # (device, B, n, int16?) -> workspace

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None, return_bounds: bool = False):
        audio = A.signal(audio, "audio", "SilenceTrimmer")
        B, n = audio.shape
        lib = L_.load()
        L_.require_device()
        dev = audio.device
        li = A.device_lengths(lengths, B, n, dev)
        pcm16 = audio.dtype == torch.int16
        out = torch.empty(B, n, dtype=torch.float32, device=dev)
        res = torch.empty(2, B, dtype=torch.int32, device=dev)           # new_len, start
        gains = torch.empty(B, dtype=torch.float32, device=dev)
        ws = self._ws.get((dev, B, n, pcm16),
                          lambda: torch.empty(int(lib.efts_trim_workspace_bytes(B, n, self.hop, int(pcm16))), dtype=torch.uint8, device=dev))
        keep = self.keep_frames if self.trim else -1
        peak = self.peak if self.peak is not None else 0.0
        fn, name, scale = A.pcm_entry(lib, "efts_trim", audio, self.max_wav_value)
        with O.stream_scope():
            L_.check(fn(audio.data_ptr(), n, li.data_ptr(), self.frame_length, self.hop, self.ratio, keep, peak, *scale, out.data_ptr(), n,
                        res[0].data_ptr(), res[1].data_ptr(), gains.data_ptr(), ws.data_ptr(), B, O._stream()), name)
        out_lengths = res[0].to(torch.int64)
        if return_bounds:
            return out, out_lengths, res[1].to(torch.int64), gains
        return out, out_lengths
