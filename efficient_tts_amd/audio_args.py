"""The host side that the audio ops share around their launches: argument checks, lengths on the device, frame counts on the host, the
choice between an entry point and its int16 twin, and the per-shape workspace cache.  Importing it needs no device."""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import numpy as np
import torch


def as_int(value, name: str) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {value!r}")
    return int(value)


def max_wav(value) -> float:
    """max_wav_value as a float: int16 PCM is scaled by its reciprocal at the kernels' loads"""
    if not float(value) > 0.0:
        raise ValueError(f"max_wav_value must be > 0, got {value!r}")
    return float(value)


def signal(t: torch.Tensor, name: str, who: Optional[str] = None) -> torch.Tensor:
    """t, contiguous, after the checks of a padded batch of samples: [B, n] with B, n >= 1, float32 or int16.  `who` names the caller in the
    refusal of a host tensor; None is for a caller that moves the samples to its device itself."""
    if t.dim() != 2 or t.dtype not in (torch.float32, torch.int16):
        raise ValueError(f"expected {name} [B, n], float32 or int16")
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name}: empty batch or no samples")
    if who is not None and not t.is_cuda:
        raise RuntimeError(f"{who} runs on an MI355X device only (no CPU path)")
    return t.contiguous()


def device_lengths(lengths: Optional[torch.Tensor], B: int, n: int, dev) -> torch.Tensor:
    """int32 [B] on `dev`: the lengths clamped to 0 .. n, or n for every item without lengths"""
    if lengths is None:
        return torch.full((B,), n, dtype=torch.int32, device=dev)
    if lengths.shape != (B,):
        raise ValueError("lengths must be [B]")
    return lengths.to(device=dev, dtype=torch.int64).clamp(0, n).to(torch.int32)


def frame_counts(lengths: torch.Tensor, n: int, hop: int, pad: int, short_ok: bool = False,
                 max_frames: Optional[int] = None) -> Tuple[List[int], List[int], int]:
    """(lh, fh, T) as plain ints from the one host copy of `lengths`: the sample counts (each at most n, the buffer), the frame counts
    l // hop and the frames of the output, max(fh) or `max_frames`.  An item no longer than `pad`, the reflect padding, is refused; with
    `short_ok` it gets 0 frames instead, and T is then at least 1.  The caller uploads [lh, fh] as one int32 [2, B] tensor."""
    lh = lengths.detach().to("cpu", torch.int64).tolist()
    if max(lh) > n:
        raise ValueError("lengths exceed the audio buffer")
    if min(lh) > pad:
        fh = [l // hop for l in lh]
    elif short_ok:
        fh = [l // hop if l > pad else 0 for l in lh]
    else:
        raise ValueError("every item must be longer than the reflect padding (n_fft - hop) / 2")
    if max_frames is None:
        return lh, fh, max(max(fh), 1) if short_ok else max(fh)
    if int(max_frames) < 1:
        raise ValueError("max_frames must be >= 1")
    return lh, fh, int(max_frames)


def pcm_entry(lib, base: str, audio: torch.Tensor, max_wav_value: float) -> Tuple[Callable, str, tuple]:
    """(fn, name, scale_args) of the entry point that reads `audio`: `base` and () for float32, `base`_pcm16 and (1 / max_wav_value,) for
    int16.  Where the scale stands among the arguments differs from entry to entry: the call site splices scale_args in."""
    if audio.dtype == torch.int16:
        return getattr(lib, base + "_pcm16"), base + "_pcm16", (1.0 / max_wav_value,)
    return getattr(lib, base), base, ()


class Cache:
    """Per-shape workspaces: get(key, make) returns the entry of `key` and calls make() for a new one.  At most `capacity` entries; a new
    key beyond that drops the oldest one by INSERTION order -- a hit does not renew its entry (this is not least-recently-used)."""

    def __init__(self, capacity: int = 5):
        self.capacity, self.entries = capacity, {}

    def get(self, key, make: Callable):
        if key not in self.entries:
            if len(self.entries) >= self.capacity:
                self.entries.pop(next(iter(self.entries)))
            self.entries[key] = make()
        return self.entries[key]

    def clear(self) -> None:
        self.entries.clear()
