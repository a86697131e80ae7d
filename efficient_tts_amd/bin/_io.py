"""Reading recordings for the command-line tools."""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch


def read_wav(path: str, wav_dir: Optional[str] = None, rate: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """(int16 samples [n], sampling rate) of a mono 16-bit PCM wav file.  A path that does not exist is looked up by its file name under
    `wav_dir`; `rate`: the sampling rate the file must have (None: any)."""
    from scipy.io.wavfile import read
    if not os.path.exists(path) and wav_dir:
        path = os.path.join(wav_dir, os.path.basename(path))
    sr, data = read(path)
    if data.dtype != np.int16 or data.ndim != 1 or (rate is not None and sr != rate):
        raise ValueError(f"{path}: expected mono 16-bit PCM" + ("" if rate is None else f" at {rate} Hz"))
    return torch.from_numpy(np.ascontiguousarray(data)), int(sr)
