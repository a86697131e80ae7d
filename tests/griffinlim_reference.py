"""Dtype-generic restatement of the Griffin-Lim vocoder (efficient_tts_amd/griffinlim.py, steps 1-6)  --  TEST INFRASTRUCTURE.

Plain torch on the CPU, written from the published algorithm (Griffin & Lim 1984; momentum: Perraudin, Balazs & Sondergaard
2013) and the conventions of the front-end: n_fft 1024, hop 256, periodic Hann, 384 samples of padding per side, no centring.
The working dtype follows the inputs: in float64 it is the reference of tests/test_griffinlim_gpu.py, in float32 its twin (the
same operations in the kernels' precision, whose deviation from float64 scales the bound).  Both use the float32 Hann window the
kernels are given, upcast.  One item at a time: a spectrum is [T, 513] complex, a padded signal [256 T + 768].
"""
from __future__ import annotations

import math

import numpy as np
import torch

N_FFT, HOP, BINS = 1024, 256, 513
PAD = (N_FFT - HOP) // 2
SR, N_MELS, FMIN, FMAX = 22050, 80, 0.0, 8000.0
MAG_FLOOR, EPS = 1e-5, 1e-8


def cplx(dtype: torch.dtype) -> torch.dtype:
    return torch.complex128 if dtype == torch.float64 else torch.complex64


def window(dtype: torch.dtype) -> torch.Tensor:
    return torch.hann_window(N_FFT, periodic=True, dtype=torch.float32).to(dtype)


def padded_len(T: int) -> int:
    return HOP * T + N_FFT - HOP


# ---------------------------------------------------------------------------------------------- analysis / synthesis
def analysis(y_pad: torch.Tensor) -> torch.Tensor:
    """padded signal [256 T + 768] -> spectrum [T, 513]: frame t starts at padded sample 256 t"""
    fr = y_pad.unfold(0, N_FFT, HOP) * window(y_pad.dtype)
    return torch.fft.rfft(fr, dim=-1)


def windowed_frames(X: torch.Tensor) -> torch.Tensor:
    """spectrum [T, 513] -> hann * irfft [T, 1024]"""
    return torch.fft.irfft(X, n=N_FFT, dim=-1) * window(X.real.dtype)


def overlap_add(wf: torch.Tensor) -> torch.Tensor:
    """windowed frames [T, 1024] -> padded signal [256 T + 768], divided by the window sum-of-squares of the frames that really cover
    each sample (1.5 in the interior, less at the edges; floor 1e-8)"""
    T = wf.shape[0]
    w2 = window(wf.dtype) ** 2
    y = torch.zeros(padded_len(T), dtype=wf.dtype)
    wss = torch.zeros_like(y)
    for k in range(N_FFT // HOP):               # quarter k of every frame: frame t puts it at 256 (t + k)
        y[HOP * k:HOP * (k + T)] += wf[:, HOP * k:HOP * (k + 1)].reshape(-1)
        wss[HOP * k:HOP * (k + T)] += w2[HOP * k:HOP * (k + 1)].repeat(T)
    return y / wss.clamp_min(EPS)


def synthesis(X: torch.Tensor) -> torch.Tensor:
    return overlap_add(windowed_frames(X))


def project(Y: torch.Tensor, Y_prev: torch.Tensor, M: torch.Tensor, momentum: float) -> torch.Tensor:
    C = Y + momentum * (Y - Y_prev)
    return C * (M / C.abs().clamp_min(EPS))


# ---------------------------------------------------------------------------------------------- step 1
def filterbank() -> np.ndarray:
    from efficient_tts_amd.frontend import slaney_mel_filterbank
    return slaney_mel_filterbank(SR, N_FFT, N_MELS, FMIN, FMAX)


def mel_to_magnitude(logmel: torch.Tensor) -> torch.Tensor:
    """logmel [80, T] -> M [T, 513] = max(pinv(FB) @ exp(logmel), 1e-5), the pseudo-inverse in float64"""
    pinv = torch.from_numpy(np.linalg.pinv(filterbank().astype(np.float64))).to(logmel.dtype)
    return (pinv @ torch.exp(logmel)).clamp_min(MAG_FLOOR).t().contiguous()


# ---------------------------------------------------------------------------------------------- step 2
def _hash_u32(x: np.ndarray) -> np.ndarray:
    """the counter-based hash of the Dropout masks (csrc/efts_internal.h, hash_u32)"""
    x = x.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return x


def initial_spectrum(M: torch.Tensor, init: str = "zero", seed: int = 0) -> torch.Tensor:
    if init == "zero":
        return M.to(cplx(M.dtype))
    T = M.shape[0]
    idx = np.arange(T * BINS, dtype=np.uint64)
    h = _hash_u32(idx ^ _hash_u32(np.array([seed & 0xFFFFFFFF])))
    u = torch.from_numpy((h >> np.uint64(8)).astype(np.float64) / 16777216.0).reshape(T, BINS)
    phi = (2.0 * math.pi * u).to(M.dtype)
    return torch.polar(M, phi)


# ---------------------------------------------------------------------------------------------- steps 3-5
def griffinlim(M: torch.Tensor, n_iter: int = 32, momentum: float = 0.99, init: str = "zero", seed: int = 0) -> torch.Tensor:
    """M [T, 513] -> padded signal [256 T + 768]"""
    X = initial_spectrum(M, init, seed)
    Y_prev = torch.zeros_like(X)
    for _ in range(n_iter):
        Y = analysis(synthesis(X))
        X = project(Y, Y_prev, M, momentum)
        Y_prev = Y
    return synthesis(X)


def trim(y_pad: torch.Tensor) -> torch.Tensor:
    return y_pad[PAD:y_pad.shape[0] - PAD]


def vocode(logmel: torch.Tensor, **kw) -> torch.Tensor:
    """logmel [80, T] -> audio [256 T]"""
    return trim(griffinlim(mel_to_magnitude(logmel), **kw))


# ---------------------------------------------------------------------------------------------- the front-end, and figures of merit
def reflect_pad(audio: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.pad(audio[None, None], (PAD, PAD), mode="reflect")[0, 0]


def logmel(audio: torch.Tensor) -> torch.Tensor:
    """audio [256 T] -> log-mel [80, T] as the front-end computes it (meldataset.py:49-82)"""
    Y = analysis(reflect_pad(audio))
    mag = torch.sqrt(Y.real ** 2 + Y.imag ** 2 + 1e-9)
    fb = torch.from_numpy(filterbank()).to(audio.dtype)
    return torch.log((fb @ mag.t()).clamp_min(1e-5))


def spectral_convergence(audio: torch.Tensor, M: torch.Tensor) -> float:
    """|| |analysis(audio)| - M ||_F / ||M||_F, audio [256 T] reflect-padded as the front-end does"""
    A = analysis(reflect_pad(audio.to(M.dtype))).abs()
    return float(torch.linalg.norm(A - M) / torch.linalg.norm(M))


# ---------------------------------------------------------------------------------------------- test signals
def voiced(seconds: float, seed: int) -> torch.Tensor:
    """seeded synthetic 'voiced' audio, float64 [256 T]: a few harmonics of a fundamental with vibrato under a slow amplitude envelope,
    plus low-level noise"""
    T = max(1, int(round(seconds * SR / HOP)))
    n = HOP * T
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / SR
    f0 = 110.0 + 90.0 * float(torch.rand(1, generator=g))
    vib = 1.0 + 0.02 * torch.sin(2.0 * math.pi * (4.0 + 2.0 * float(torch.rand(1, generator=g))) * t)
    phase = 2.0 * math.pi * torch.cumsum(f0 * vib, 0) / SR
    y = torch.zeros(n, dtype=torch.float64)
    for h in range(1, 9):
        y += (0.6 ** (h - 1)) * (0.5 + float(torch.rand(1, generator=g))) * torch.sin(h * phase + 6.28 * float(torch.rand(1, generator=g)))
    env = 0.15 + 0.85 * torch.sin(math.pi * (t * (1.5 + float(torch.rand(1, generator=g)))) % math.pi) ** 2
    y = y * env
    y = 0.5 * y / y.abs().max() + 1e-3 * torch.randn(n, generator=g, dtype=torch.float64)
    return y
