"""On-device pitch tracking: YIN (de Cheveigne & Kawahara 2002) on the frame grid of `LogMelFrontend`, so that f0[b, t] belongs to mel[b, t].

Item b has lengths[b] // hop frames; frame t covers samples t hop - pad .. t hop - pad + n_fft - 1 with pad = (n_fft - hop) / 2, reflected at
the item's ends.  Per frame x, with W = n_fft / 2, tau_min = floor(sr / fmax) and tau_max = floor(sr / fmin) <= W:

    d(tau)  = sum_{j < W} (x[j] - x[j + tau])^2                       (the direct form, fp32 fused multiply-adds, j ascending)
    d'(tau) = d(tau) tau / (d(1) + .. + d(tau)), 1 where that sum is 0
    tau     = the smallest lag in [tau_min, tau_max - 1] with d'(tau) < threshold, advanced while d' keeps falling, refined by a parabola
              through d'(tau - 1), d'(tau), d'(tau + 1) (shift clamped to [-1, 1]);  f0 = sr / tau, or 0 when no lag is under the threshold

One launch (csrc/efts_pitch.hip, `efts_yin` / `efts_yin_pcm16`); include/efts_abi.h states every order of summation.  fp32, no atomics: an
item gives the same bits alone, in any batch position and in any run.  No CPU path: the HIP library is required.

YIN decides every frame alone, and its rule -- the first lag under the threshold -- flips an octave up wherever the second harmonic is briefly
strong.  `ViterbiSmoother` (`PitchTracker(..., smooth=True)`) replaces the per-frame decision by the cheapest path over all lags of all frames
of an item, on the same d' (csrc/efts_pitch_viterbi.hip, `efts_f0_viterbi`).  States: the lags tau_min .. tau_max - 1 and "unvoiced".  With
Q = 65536 and lg[k] = rint(log2(k) Q), all in integers:

    voiced state k at frame t costs  q(d'(t, k)) + (octave_cost_q (lg[k] - lg[tau_min]) >> 16),  q(x) = rint(x Q) clipped at 4 Q;  unvoiced: unvoiced_cost_q
    a step k' -> k costs (jump_cost_q |lg[k] - lg[k']|) >> 16, voiced <-> unvoiced vuv_cost_q, unvoiced -> unvoiced nothing
    ties go to the lowest state; f0 is YIN's parabola at the path's lag (no walk to a local minimum), 0 for an unvoiced frame

The recurrence holds no floating point, so the path has one right answer (tests/viterbi_reference.py restates it in int64 and the GPU tests
demand equality).  One more launch, one workgroup per item; nothing is read back.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from . import audio_args as A
from . import lib as L
from . import ops as O

N_FFTS = (512, 1024, 2048)


def lag_range(sampling_rate: int, n_fft: int, fmin: float, fmax: float):
    """(tau_min, tau_max) as the library computes them -- floor(sr / fmax), floor(sr / fmin) in float64 on the fp32 values of fmin and fmax --
    or ValueError where the library would refuse"""
    lo = math.floor(sampling_rate / float(np.float32(fmax))) if fmax > 0 else 0
    hi = math.floor(sampling_rate / float(np.float32(fmin))) if fmin > 0 else 0
    if not (fmin > 0 and fmax > fmin and lo >= 2 and hi <= n_fft // 2 and lo < hi - 1):
        raise ValueError(f"need 0 < fmin < fmax with 2 <= floor(sr / fmax) < floor(sr / fmin) - 1 and floor(sr / fmin) <= n_fft / 2; "
                         f"got lags {lo} .. {hi} for n_fft {n_fft} (fmin {fmin}, fmax {fmax}, sr {sampling_rate})")
    return lo, hi


Q16 = 65536
MAX_COST = 16.0                                                # efts_f0_viterbi refuses a cost above 16 Q
MAX_LAG = 1024                                                 # EFTS_VITERBI_MAX_LAG

_lg_tables: Dict[tuple, torch.Tensor] = {}
_workspaces = A.Cache(capacity=5)                              # the back-pointers of the smoother, per (device, B, T, tau_min, tau_max)


def log2_table(tau_max: int) -> torch.Tensor:
    """int32 [tau_max + 1]: lg[k] = rint(log2(k) * 65536) for k >= 1 in float64 (entry 0 is never read)"""
    lg = np.zeros(tau_max + 1, dtype=np.int32)
    lg[1:] = np.rint(np.log2(np.arange(1, tau_max + 1, dtype=np.float64)) * Q16).astype(np.int32)
    return torch.from_numpy(lg)


def cost_q16(name: str, value: float) -> int:
    if not 0.0 <= float(value) <= MAX_COST:
        raise ValueError(f"{name} must lie in 0 .. {MAX_COST:g} (got {value})")
    return int(np.rint(np.float64(value) * Q16))


class ViterbiSmoother:
    """f0, aperiodicity, lag = ViterbiSmoother(device, sampling_rate, tau_min, tau_max)(cmnd, frames)

    cmnd: [B, T, tau_max + 1] float32 on the device, every d'(tau) as `PitchTracker(..., return_cmnd=True)` returns it (any item and frame
    stride, the lags contiguous); frames: [B] frame counts.  Returns f0 [B, T] in Hz (0: unvoiced), aperiodicity [B, T] (d' at the path's lag,
    or the row's minimum for an unvoiced frame) and lag [B, T] int32 (0: unvoiced); all three are 0 at or beyond an item's count.  The four
    costs are in units of d'.  The lg table and the back-pointer workspace (T (tau_max - tau_min + 1) uint16 per item) are cached; the calls on
    one stream share the workspace.  Nothing is read back."""

    def __init__(self, device, sampling_rate: int, tau_min: int, tau_max: int, unvoiced_cost: float = 0.15, octave_cost: float = 0.02,
                 jump_cost: float = 0.35, vuv_cost: float = 0.14):
        self.dev = torch.device(device)
        self.sr, self.tau_min, self.tau_max = int(sampling_rate), int(tau_min), int(tau_max)
        if not (2 <= self.tau_min < self.tau_max - 1 and self.tau_max <= MAX_LAG) or self.sr < 1:
            raise ValueError(f"need 2 <= tau_min < tau_max - 1, tau_max <= {MAX_LAG} and sampling_rate >= 1 (got lags {tau_min} .. {tau_max})")
        self.costs_q = tuple(cost_q16(name, v) for name, v in (("unvoiced_cost", unvoiced_cost), ("octave_cost", octave_cost),
                                                               ("jump_cost", jump_cost), ("vuv_cost", vuv_cost)))
        L.load()
        L.require_device()
        key = (self.dev, self.tau_max)
        if key not in _lg_tables:
            _lg_tables[key] = log2_table(self.tau_max).to(self.dev)
        self.lg = _lg_tables[key]

    @torch.no_grad()
    def __call__(self, cmnd: torch.Tensor, frames: torch.Tensor):
        if cmnd.dim() != 3 or cmnd.dtype != torch.float32 or cmnd.shape[0] < 1 or cmnd.shape[1] < 1 or cmnd.shape[2] != self.tau_max + 1:
            raise ValueError(f"cmnd must be float32 [B, T, {self.tau_max + 1}]")
        if not cmnd.is_cuda:
            raise RuntimeError("efficient_tts_amd.pitch runs on an MI355X device only (no CPU path)")
        B, T = cmnd.shape[0], cmnd.shape[1]
        if frames.shape != (B,):
            raise ValueError("frames must be [B]")
        if cmnd.stride(2) != 1 or cmnd.stride(1) < cmnd.shape[2] or cmnd.stride(0) < 0:
            cmnd = cmnd.contiguous()
        fr = frames.to(device=cmnd.device, dtype=torch.int32)
        lib = L.load()
        need = int(lib.efts_f0_viterbi_workspace_bytes(T, self.tau_min, self.tau_max))
        if need <= 0:
            raise ValueError(f"ViterbiSmoother: {T} frames are more than one call takes")
        ws = _workspaces.get((self.dev, B, T, self.tau_min, self.tau_max), lambda: torch.empty(B * need, dtype=torch.uint8, device=self.dev))
        f0 = torch.empty(B, T, dtype=torch.float32, device=cmnd.device)
        ap = torch.empty(B, T, dtype=torch.float32, device=cmnd.device)
        lag = torch.empty(B, T, dtype=torch.int32, device=cmnd.device)
        with O.stream_scope():
            L.check(lib.efts_f0_viterbi(cmnd.data_ptr(), cmnd.stride(0), cmnd.stride(1), fr.data_ptr(), self.lg.data_ptr(), f0.data_ptr(), ap.data_ptr(),
                                        lag.data_ptr(), ws.data_ptr(), ws.numel(), B, T, self.tau_min, self.tau_max, self.sr, *self.costs_q, O._stream()),
                    "efts_f0_viterbi")
        return f0, ap, lag


class PitchTracker:
    """f0, aperiodicity, frames = PitchTracker(device)(audio, lengths)

    audio: [B, L] float32 in [-1, 1] or int16 PCM (scaled by 1 / max_wav_value at the kernel's loads), on the device or the host; lengths: [B]
    sample counts.  Returns f0 [B, T] in Hz (0: unvoiced, and frames at or beyond an item's count), aperiodicity [B, T] (d' at the chosen
    lag, or its minimum over the search range for an unvoiced frame: apply a threshold of your own to it) and frames [B] int64;
    T = max frames or `max_frames`.  `return_cmnd=True` appends cmnd [B, T, tau_max + 1], every d'(tau).  `short_ok=True` gives an item no
    longer than the reflect padding zero frames instead of refusing it.

    `smooth=True` (keyword only, with the four costs of `ViterbiSmoother`) decides the frames of an item together: YIN writes every d', and f0 and
    aperiodicity are those of the cheapest path over the lags (`threshold` then plays no part).  The tuple keeps its shape.  `smooth=False` is the
    tracker as it was, bit for bit, with no further launch or allocation."""

    def __init__(self, device, sampling_rate: int = 22050, n_fft: int = 1024, hop_size: int = 256, fmin: float = 60.0, fmax: float = 600.0,
                 threshold: float = 0.15, max_wav_value: float = 32768.0, *, smooth: bool = False, unvoiced_cost: float = 0.15,
                 octave_cost: float = 0.02, jump_cost: float = 0.35, vuv_cost: float = 0.14):
        if n_fft not in N_FFTS:
            raise ValueError(f"n_fft must be one of {N_FFTS}")
        if not 1 <= hop_size <= n_fft or (n_fft - hop_size) % 2:
            raise ValueError("hop_size must lie in 1 .. n_fft with n_fft - hop_size even")
        if not threshold > 0:
            raise ValueError("threshold must be > 0")
        self.max_wav_value = A.max_wav(max_wav_value)
        self.tau_min, self.tau_max = lag_range(int(sampling_rate), n_fft, fmin, fmax)
        self.dev = torch.device(device)
        self.sr, self.n_fft, self.hop, self.pad = int(sampling_rate), int(n_fft), int(hop_size), (n_fft - hop_size) // 2
        self.fmin, self.fmax, self.threshold = float(fmin), float(fmax), float(threshold)
        L.load()
        L.require_device()
        self.smoother = ViterbiSmoother(self.dev, self.sr, self.tau_min, self.tau_max, unvoiced_cost, octave_cost, jump_cost, vuv_cost) if smooth else None

    def frames_of(self, lengths: torch.Tensor) -> torch.Tensor:
        return torch.div(lengths.to(torch.int64), self.hop, rounding_mode="floor")

    @torch.no_grad()
    def __call__(self, audio: torch.Tensor, lengths: torch.Tensor, max_frames: Optional[int] = None, return_cmnd: bool = False, short_ok: bool = False):
        audio = A.signal(audio.to(self.dev), "audio", "efficient_tts_amd.pitch")
        B = audio.shape[0]
        if lengths.shape != (B,):
            raise ValueError("lengths must be [B]")
        lh, fh, T = A.frame_counts(lengths, audio.shape[1], self.hop, self.pad, short_ok, max_frames)   # the one host copy: the checks run on plain ints
        both = torch.tensor([lh, fh], dtype=torch.int32).to(self.dev, non_blocking=True)
        f0 = torch.empty(B, T, dtype=torch.float32, device=self.dev)
        ap = torch.empty(B, T, dtype=torch.float32, device=self.dev)
        cmnd = torch.empty(B, T, self.tau_max + 1, dtype=torch.float32, device=self.dev) if return_cmnd or self.smoother else None
        fn, name, scale = A.pcm_entry(L.load(), "efts_yin", audio, self.max_wav_value)
        with O.stream_scope():
            L.check(fn(audio.data_ptr(), audio.shape[1], *scale, both[0].data_ptr(), f0.data_ptr(), ap.data_ptr(), O._p(cmnd), B, T, self.n_fft, self.hop,
                       self.sr, self.fmin, self.fmax, self.threshold, O._stream()), name)
        if self.smoother is not None:
            f0, ap, _ = self.smoother(cmnd, both[1])
        frames = both[1].to(torch.int64)
        return (f0, ap, frames, cmnd) if return_cmnd else (f0, ap, frames)
