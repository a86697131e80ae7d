"""Scoring synthesised speech against a recording on the device: mel-cepstral distortion (MCD) along a dynamic-time-warping (DTW) path.

A free-running mel has its own length, so it is compared with the recording's log-mel after time alignment:

    c[t][k-1] = sum over n of sqrt(2 / N) cos(pi k (n + 1/2) / N) mel[t][n],  k = 1 .. n_coef      (orthonormal DCT-II without c0: loudness does not count)
    d(i, j)   = || c_a[i] - c_b[j] ||_2
    A(0, 0) = d(0, 0), A(i, j) = d(i, j) + min(A(i-1, j-1), A(i-1, j), A(i, j-1)), every step of weight 1;  L = cells on the chosen path
    (ties: the diagonal, then (i-1, j), then (i, j-1); a later one wins only when strictly smaller)
    mcd = (10 / ln 10) sqrt(2) A(last, last) / L(last, last)   dB

`dtw_path` returns the chosen path itself (`efts_dtw_path`: the same kernel body records every cell's move in a workspace and walks them back
inside the launch), `MelCepstralDistortion(...)(..., return_path=True)` passes it on, and `F0Error` reads two F0 contours (`pitch.PitchTracker`)
along it: the F0 error in cents on the cells voiced on both sides, and the share of cells whose voicing differs.

The DCT table is computed once on the host in float64 and kept as fp32 in device memory; the sums and the recurrence run in
csrc/efts_score.hip (`efts_mel_cepstrum`, `efts_dtw`): fp32, one fixed order, no atomics, no cost matrix in memory.  An item gives the same
bits alone, in any batch and in any run.  No CPU path: the HIP library is required.

The mels are this project's own natural-log mels (`LogMelFrontend`, the model's output).  The numbers therefore compare checkpoints of
this project with each other; they are NOT comparable to MCDs computed from SPTK mel-cepstra of waveforms.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np
import torch

from . import lib as L_
from . import ops as O
from .audio_args import Cache

MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)
MAX_MELS, MAX_COEF = 128, 32                                      # limits of efts_mel_cepstrum (include/efts_abi.h)

_tables: Dict[tuple, torch.Tensor] = {}
_workspaces = Cache(capacity=5)                                    # the move record of dtw_path, per (device, B, Tx, Ty)


def dct_table(n_mels: int, n_coef: int) -> torch.Tensor:
    """fp32 [n_coef, n_mels]: table[k-1][n] = sqrt(2 / N) cos(pi k (n + 1/2) / N), k = 1 .. n_coef, float64 rounded once"""
    if not 1 <= n_coef <= MAX_COEF or not 1 <= n_mels <= MAX_MELS or n_coef >= n_mels:
        raise ValueError(f"need 1 <= n_coef <= {MAX_COEF}, n_coef < n_mels <= {MAX_MELS}, got n_coef {n_coef}, n_mels {n_mels}")
    k = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
    n = np.arange(n_mels, dtype=np.float64)[None, :]
    return torch.from_numpy((math.sqrt(2.0 / n_mels) * np.cos(math.pi * k * (n + 0.5) / n_mels)).astype(np.float32)).contiguous()


def _table_on(dev: torch.device, n_mels: int, n_coef: int) -> torch.Tensor:
    key = (dev, n_mels, n_coef)
    if key not in _tables:
        _tables[key] = dct_table(n_mels, n_coef).to(dev)
    return _tables[key]


def _rows(name: str, t: torch.Tensor, lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """a padded fp32 batch [B, T, D] whose rows are contiguous (any row and item stride), and its lengths as int32 on the same device
    (lengths already there are used in place; host lengths cost one small host-to-device copy per call)"""
    if t.dim() != 3 or t.dtype != torch.float32 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name}: expected a float32 batch [B, T, D]")
    if not t.is_cuda:
        raise RuntimeError("efficient_tts_amd.score runs on an MI355X device only (no CPU path)")
    if lengths.shape != (t.shape[0],):
        raise ValueError(f"{name}: lengths must be [B]")
    if t.stride(2) != 1 or t.stride(1) < t.shape[2] or t.stride(0) < 0:
        t = t.contiguous()
    return t, lengths.to(device=t.device, dtype=torch.int32)


def _cepstrum(mel: torch.Tensor, lengths: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    mel, li = _rows("mel", mel, lengths)
    B, T, n_mels = mel.shape
    n_coef = table.shape[0]
    if table.shape[1] != n_mels:
        raise ValueError(f"expected mels [B, T, {table.shape[1]}]")
    lib = L_.load()
    L_.require_device()
    out = torch.empty(B, T, n_coef, dtype=torch.float32, device=mel.device)
    with O.stream_scope():
        L_.check(lib.efts_mel_cepstrum(mel.data_ptr(), mel.stride(1), mel.stride(0), li.data_ptr(), table.data_ptr(), out.data_ptr(), B, T, n_mels,
                                       n_coef, O._stream()), "efts_mel_cepstrum")
    return out


@torch.no_grad()
def mel_cepstrum(mel: torch.Tensor, lengths: torch.Tensor, n_coef: int = 13) -> torch.Tensor:
    """log-mel [B, T, n_mels] -> mel-cepstra [B, T, n_coef] (c1 .. c_n_coef); rows at or beyond lengths[b] are zeros and are not read"""
    if mel.dim() != 3:
        raise ValueError("mel: expected a float32 batch [B, T, n_mels]")
    return _cepstrum(mel, lengths, _table_on(mel.device, mel.shape[2], int(n_coef)))


@torch.no_grad()
def dtw(x: torch.Tensor, x_lengths: torch.Tensor, y: torch.Tensor, y_lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(cost [B] fp32, path_len [B] int32) of the cheapest warping path between x[b, :x_lengths[b]] and y[b, :y_lengths[b]], x [B, Tx, D],
    y [B, Ty, D], D <= 32, Tx and Ty <= 8192.  Rows beyond an item's length are never read; an item with a length below 1 gets
    (NaN, 0).  The path itself is not returned."""
    x, xl = _rows("x", x, x_lengths)
    y, yl = _rows("y", y, y_lengths)
    if y.shape[0] != x.shape[0] or y.shape[2] != x.shape[2] or y.device != x.device:
        raise ValueError("x and y must agree in B, D and device")
    B, Tx, D = x.shape
    lib = L_.load()
    L_.require_device()
    cost = torch.empty(B, dtype=torch.float32, device=x.device)
    path_len = torch.empty(B, dtype=torch.int32, device=x.device)
    with O.stream_scope():
        L_.check(lib.efts_dtw(x.data_ptr(), x.stride(1), x.stride(0), xl.data_ptr(), Tx, y.data_ptr(), y.stride(1), y.stride(0), yl.data_ptr(),
                              y.shape[1], D, cost.data_ptr(), path_len.data_ptr(), B, O._stream()), "efts_dtw")
    return cost, path_len


@torch.no_grad()
def dtw_path(x: torch.Tensor, x_lengths: torch.Tensor, y: torch.Tensor, y_lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(cost [B] fp32, path_len [B] int32, path [B, Tx + Ty - 1, 2] int32): `dtw`'s cost and path_len, bit for bit, and the path itself.
    path[b, k] = (i, j) is the k-th cell in forward order, from (0, 0) to (x_lengths[b] - 1, y_lengths[b] - 1); rows at and beyond
    path_len[b] are not written (they hold whatever the allocation held).  The move record lives in a workspace of
    ceil(Tx / 1024) (Ty + 255) 256 bytes per pair, cached per (device, B, Tx, Ty) and shared by the calls on one stream."""
    x, xl = _rows("x", x, x_lengths)
    y, yl = _rows("y", y, y_lengths)
    if y.shape[0] != x.shape[0] or y.shape[2] != x.shape[2] or y.device != x.device:
        raise ValueError("x and y must agree in B, D and device")
    B, Tx, D = x.shape
    Ty = y.shape[1]
    lib = L_.load()
    L_.require_device()
    need = int(lib.efts_dtw_path_workspace_bytes(Tx, Ty))
    if need <= 0:
        raise ValueError(f"dtw_path: Tx and Ty must be 1 .. 8192 frames (got {Tx}, {Ty})")
    ws = _workspaces.get((x.device, B, Tx, Ty), lambda: torch.empty(B * need, dtype=torch.uint8, device=x.device))
    cost = torch.empty(B, dtype=torch.float32, device=x.device)
    path_len = torch.empty(B, dtype=torch.int32, device=x.device)
    path = torch.empty(B, Tx + Ty - 1, 2, dtype=torch.int32, device=x.device)
    with O.stream_scope():
        L_.check(lib.efts_dtw_path(x.data_ptr(), x.stride(1), x.stride(0), xl.data_ptr(), Tx, y.data_ptr(), y.stride(1), y.stride(0), yl.data_ptr(),
                                   Ty, D, cost.data_ptr(), path_len.data_ptr(), path.data_ptr(), ws.data_ptr(), ws.numel(), B, O._stream()), "efts_dtw_path")
    return cost, path_len, path


class F0Error:
    """F0Error(device)(f0_a [B, Ta], f0_b [B, Tb], path [B, P, 2] int32, path_len [B]) -> dict of device tensors, nothing read back:
    `voiced_pairs` [B] int32, the path cells voiced (f0 > 0) on both sides; `f0_rmse_cents` [B] = sqrt(mean over those cells of
    (1200 log2(f0_a / f0_b))^2), NaN without such a cell; `vuv_error` [B], the share of path cells whose voicing differs, NaN for an empty path."""

    def __init__(self, device):
        self.dev = torch.device(device)

    @torch.no_grad()
    def __call__(self, f0_a: torch.Tensor, f0_b: torch.Tensor, path: torch.Tensor, path_len: torch.Tensor) -> Dict[str, torch.Tensor]:
        for name, f in (("f0_a", f0_a), ("f0_b", f0_b)):
            if f.dim() != 2 or f.dtype != torch.float32 or f.shape[0] != f0_a.shape[0] or f.shape[1] < 1:
                raise ValueError(f"{name}: expected float32 [B, T]")
        B = f0_a.shape[0]
        if path.dim() != 3 or path.shape[0] != B or path.shape[1] < 1 or path.shape[2] != 2 or path.dtype != torch.int32 or path_len.shape != (B,):
            raise ValueError("expected path [B, P, 2] int32 and path_len [B]")
        if not f0_a.is_cuda:
            raise RuntimeError("efficient_tts_amd.score runs on an MI355X device only (no CPU path)")
        f0_a, f0_b, path = f0_a.contiguous(), f0_b.to(f0_a.device).contiguous(), path.to(f0_a.device).contiguous()
        pl = path_len.to(device=f0_a.device, dtype=torch.int32)
        lib = L_.load()
        L_.require_device()
        rmse = torch.empty(B, dtype=torch.float32, device=f0_a.device)
        vuv = torch.empty(B, dtype=torch.float32, device=f0_a.device)
        pairs = torch.empty(B, dtype=torch.int32, device=f0_a.device)
        with O.stream_scope():
            L_.check(lib.efts_f0_path_error(f0_a.data_ptr(), f0_a.stride(0), f0_a.shape[1], f0_b.data_ptr(), f0_b.stride(0), f0_b.shape[1], path.data_ptr(),
                                            path.shape[1], pl.data_ptr(), rmse.data_ptr(), vuv.data_ptr(), pairs.data_ptr(), B, O._stream()),
                     "efts_f0_path_error")
        return dict(f0_rmse_cents=rmse, vuv_error=vuv, voiced_pairs=pairs)


class MelCepstralDistortion:
    """MelCepstralDistortion(device, num_mels=80, n_coef=13)(mel_a [B, Ta, num_mels], len_a [B], mel_b [B, Tb, num_mels], len_b [B]) -> dict of
    device tensors: `mcd` [B] in dB = (10 / ln 10) sqrt(2) cost / path_len, `cost` and `path_len` as `dtw` returns them for the two
    mel-cepstra, `frames_ratio` [B] = len_a / len_b with the lengths clamped to the padded sizes as the kernels clamp them.  An item with
    a length below 1 on either side has no path: its `mcd`, `cost` and `frames_ratio` are NaN and its `path_len` 0 -- a caller that averages
    leaves such items out (bin/score.py does).  Three launches; nothing is read back, and with the lengths on the device nothing is copied.
    `return_path=True` runs `dtw_path` in the place of `dtw` and adds `path` [B, Ta + Tb - 1, 2]; every other entry keeps its bits.

    The mels are this project's natural-log mels: the numbers compare checkpoints of this project with each other and are not comparable
    to MCDs computed from SPTK cepstra of waveforms.  `efficient_tts_amd.mcep.WaveformMCD` computes the literature's number, from
    order-24 all-pass-warped mel-cepstra of the two waveforms."""

    def __init__(self, device, num_mels: int = 80, n_coef: int = 13):
        self.dev = torch.device(device)
        self.num_mels, self.n_coef = int(num_mels), int(n_coef)
        self.table = _table_on(self.dev, self.num_mels, self.n_coef)

    @torch.no_grad()
    def __call__(self, mel_a: torch.Tensor, len_a: torch.Tensor, mel_b: torch.Tensor, len_b: torch.Tensor, *,
                 return_path: bool = False) -> Dict[str, torch.Tensor]:
        extra = {}
        if return_path:
            cost, path_len, extra["path"] = dtw_path(_cepstrum(mel_a, len_a, self.table), len_a, _cepstrum(mel_b, len_b, self.table), len_b)
        else:
            cost, path_len = dtw(_cepstrum(mel_a, len_a, self.table), len_a, _cepstrum(mel_b, len_b, self.table), len_b)
        la = len_a.to(device=cost.device, dtype=torch.float32).clamp(max=mel_a.shape[1])
        lb = len_b.to(device=cost.device, dtype=torch.float32).clamp(max=mel_b.shape[1])
        ratio = torch.where((la >= 1) & (lb >= 1), la / lb, torch.full_like(la, float("nan")))
        return dict(mcd=MCD_DB * cost / path_len, cost=cost, path_len=path_len, frames_ratio=ratio, **extra)
