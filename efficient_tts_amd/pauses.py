"""On-device shortening of the long pauses INSIDE the recordings of a padded batch: what `sox silence -l` or an aligner-based pruning pass
does offline, as one step of the device-side data path (behind `SilenceTrimmer`, in front of the level and of `LogMelFrontend`).

With the trimmer's frames (frame length W, hop H, r = 10^(top_db / 10); frame t is sound iff (double) E_t * r > (double) E_max) and
chunk c = samples c H .. c H + H - 1, quiet iff frame c is not sound:

    a pause is a maximal run of quiet chunks [c0, c1) between the first and the last sound frame (the quiet ends are the trimmer's)
    M = max(1, round(max_pause_ms * sampling_rate / (1000 H))) chunks
    a pause of n > M chunks keeps its first (M + 1) / 2 and its last M / 2 chunks; the n - M chunks between them go
    the last `fade` kept samples in front of the joint run linearly into what follows it:  x_a + w_k (x_b - x_a),  w_k = (k + 0.5) / fade
    every other kept sample keeps its bits; new_len = len - removed; chunk_src[j] = the source chunk of output chunk j, -1 behind

include/efts_abi.h has the full definition.  The plan and the copy run in csrc/efts_pauses.hip (`efts_pauses`, `efts_pauses_pcm16`): three
launches, no atomics, nothing read back by the host.  No CPU path: the HIP library is required.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import audio_args as A
from . import lib as L_
from . import ops as O
from .trim import FRAME_LENGTHS


def fade_table(fade: int) -> np.ndarray:
    """w_k = (k + 0.5) / fade for k = 0 .. fade - 1: float64, rounded once to float32"""
    fade = A.as_int(fade, "fade")
    if fade < 0:
        raise ValueError(f"fade must be >= 0, got {fade!r}")
    return ((np.arange(fade, dtype=np.float64) + 0.5) / np.float64(max(fade, 1))).astype(np.float32)


def pause_chunks(max_pause_ms: float, sampling_rate: int, hop_size: int) -> int:
    """M, the longest pause in hop chunks that is kept whole: max(1, round(max_pause_ms * sampling_rate / (1000 hop_size))), halves to even"""
    return max(1, int(round(float(max_pause_ms) * int(sampling_rate) / (1000.0 * int(hop_size)))))


class PauseShortener(torch.nn.Module):
    """out, out_lengths = PauseShortener(device, sampling_rate, max_pause_ms, frame_length, hop_size, top_db, fade)(audio [B, n] float32 | int16, lengths=None)

    out: fp32 [B, n], every item compacted to the front of its row and exactly zero behind its new length; out_lengths: int64 [B].  With
    `return_stats=True` also a dict: removed int64 [B] (samples, a multiple of hop_size), pauses int64 [B] (the runs that were shortened)
    and chunk_src int32 [B, ceil(n / hop_size)] (the source chunk of every output chunk, -1 behind the last one).  int16 PCM is scaled by
    1 / max_wav_value.  Every item is treated exactly as if it had been passed alone; the call can be captured in a graph."""

    def __init__(self, device=None, sampling_rate: int = 22050, max_pause_ms: float = 300.0, frame_length: int = 1024, hop_size: int = 256,
                 top_db: float = 40.0, fade: int = 64, max_wav_value: float = 32768.0):
        super().__init__()
        self.dev = None if device is None else torch.device(device)
        self.sampling_rate = A.as_int(sampling_rate, "sampling_rate")
        if self.sampling_rate < 1:
            raise ValueError(f"sampling_rate must be >= 1, got {sampling_rate!r}")
        self.frame_length, self.hop = A.as_int(frame_length, "frame_length"), A.as_int(hop_size, "hop_size")
        if self.frame_length not in FRAME_LENGTHS:
            raise ValueError(f"frame_length must be one of {FRAME_LENGTHS}, got {frame_length!r}")
        if not 1 <= self.hop <= self.frame_length or (self.frame_length - self.hop) % 2:
            raise ValueError(f"hop_size must lie in 1 .. frame_length with frame_length - hop_size even, got {hop_size!r}")
        self.top_db = float(top_db)
        if not self.top_db > 0.0 or not np.isfinite(self.top_db):
            raise ValueError(f"top_db must be > 0, got {top_db!r}")
        if isinstance(max_pause_ms, bool) or not float(max_pause_ms) > 0.0 or not np.isfinite(float(max_pause_ms)):
            raise ValueError(f"max_pause_ms must be > 0, got {max_pause_ms!r}")
        self.max_pause_ms = float(max_pause_ms)
        self.fade = A.as_int(fade, "fade")
        if not 0 <= self.fade <= self.hop:
            raise ValueError(f"fade must lie in 0 .. hop_size, got {fade!r}")
        self.max_wav_value = A.max_wav(max_wav_value)
        self.ratio = float(10.0 ** (np.float64(self.top_db) / 10.0))        # r, float64, once
        if not self.ratio > 1.0 or not np.isfinite(self.ratio):
            raise ValueError(f"top_db {top_db!r} gives no usable threshold ratio")
        self.chunks = pause_chunks(self.max_pause_ms, self.sampling_rate, self.hop)      # M
        if self.chunks > 1 << 30:
            raise ValueError(f"max_pause_ms {max_pause_ms!r} is {self.chunks} hops: more than any item holds")
        self._table = torch.from_numpy(fade_table(self.fade))
        self._tables = A.Cache(capacity=2)   # device -> the fade table there
        self._ws = A.Cache(capacity=5)       # (device, B, n, int16?) -> workspace

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, lengths: Optional[torch.Tensor] = None, return_stats: bool = False):
        audio = A.signal(audio, "audio", "PauseShortener")
        B, n = audio.shape
        lib = L_.load()
        L_.require_device()
        dev = audio.device
        li = A.device_lengths(lengths, B, n, dev)
        pcm16 = audio.dtype == torch.int16
        t_max = -(-n // self.hop)
        out = torch.empty(B, n, dtype=torch.float32, device=dev)
        res = torch.empty(3, B, dtype=torch.int32, device=dev)           # new_len, removed, pauses
        chunk_src = torch.empty(B, t_max, dtype=torch.int32, device=dev)
        table = self._tables.get(dev, lambda: self._table.to(dev))
        ws = self._ws.get((dev, B, n, pcm16),
                          lambda: torch.empty(int(lib.efts_pauses_workspace_bytes(B, n, self.hop, int(pcm16))), dtype=torch.uint8, device=dev))
        fn, name, scale = A.pcm_entry(lib, "efts_pauses", audio, self.max_wav_value)
        with O.stream_scope():
            L_.check(fn(audio.data_ptr(), n, li.data_ptr(), self.frame_length, self.hop, self.ratio, self.chunks, self.fade,
                        table.data_ptr() if self.fade else None, *scale, out.data_ptr(), n, res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(),
                        chunk_src.data_ptr(), ws.data_ptr(), B, O._stream()), name)
        out_lengths = res[0].to(torch.int64)
        if return_stats:
            return out, out_lengths, {"removed": res[1].to(torch.int64), "pauses": res[2].to(torch.int64), "chunk_src": chunk_src}
        return out, out_lengths
