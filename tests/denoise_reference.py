"""The definition of the bias denoiser (include/efts_abi.h, "Spectral denoiser for a vocoder's bias noise") in numpy float64: a plain loop
over the frames and np.fft.  Also the inputs that the CPU and GPU tests share, and the same pipeline through torch.stft / torch.istft."""
import numpy as np

N, H, BINS = 1024, 256, 513
LD = 16384
LENGTHS = (0, 512, 513, 1024, 2049, 2304, 12345)         # 12345 = three of the kernel's runs of 16 hops (4096 samples) and 57 samples
STRENGTHS = (0.0, 0.5, 5.0)
TORCH_LENGTHS = (513, 700, 1024, 2049, 2304, 12345, 40000)


def window() -> np.ndarray:
    """periodic Hann, float64, rounded once to fp32 (what the device is given), as float64"""
    i = np.arange(N, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / N)).astype(np.float32).astype(np.float64)


def reflect(i: np.ndarray, length: int) -> np.ndarray:
    i = np.where(i < 0, -i, i)
    return np.where(i >= length, 2 * (length - 1) - i, i)


def frame_count(length: int) -> int:
    return 1 + length // H if length > N // 2 else 0


def denoise(x, bias, strength: float, stats=None) -> np.ndarray:
    """x [len] -> out [len], float64.  stats: a dict that receives `cells` and `clamped` (the (frame, bin) cells with d <= 0)"""
    x = np.asarray(x, dtype=np.float64)
    length = x.shape[0]
    T = frame_count(length)
    if T == 0:
        return x.copy()
    w = window()
    sb = float(strength) * np.asarray(bias, dtype=np.float64)
    num, den = np.zeros(length + 2 * N), np.zeros(length + 2 * N)          # index s + 512
    clamped = 0
    for t in range(T):
        idx = reflect(H * t - N // 2 + np.arange(N), length)
        X = np.fft.rfft(w * x[idx])
        m = np.abs(X)
        d = m - sb
        g = np.where(d > 0, d / np.where(m > 0, m, 1.0), 0.0)
        clamped += int((d <= 0).sum())
        Y = g * X
        Y[0], Y[-1] = Y[0].real, Y[-1].real
        y = np.fft.irfft(Y, N)
        num[H * t:H * t + N] += w * y
        den[H * t:H * t + N] += w * w
    if stats is not None:
        stats["cells"], stats["clamped"] = T * BINS, clamped
    return (num / np.maximum(den, 1e-8))[N // 2:N // 2 + length]


def denoise_torch(x, bias, strength: float, dtype):
    """the same through torch.stft -> gain -> torch.istft on the CPU at `dtype` (float64: the check of the reference; float32: the yardstick
    for the device's error)"""
    import torch
    xt = torch.as_tensor(np.asarray(x), dtype=dtype)
    if xt.shape[0] <= N // 2:
        return xt.numpy().astype(np.float64)
    w = torch.as_tensor(window(), dtype=dtype)
    X = torch.stft(xt, N, H, N, window=w, center=True, pad_mode="reflect", return_complex=True)
    m = X.abs()
    d = m - torch.as_tensor(float(strength) * np.asarray(bias, dtype=np.float64), dtype=dtype)[:, None]
    g = torch.where(d > 0, d / torch.where(m > 0, m, torch.ones_like(m)), torch.zeros_like(m))
    return torch.istft(X * g, N, H, N, window=w, center=True, length=xt.shape[0]).numpy().astype(np.float64)


def signal(length: int, seed: int) -> np.ndarray:
    """0.3 sin(2 pi 220 t) + 0.05 * noise at 22 050 Hz, fp32"""
    rng = np.random.default_rng(seed)
    t = np.arange(length, dtype=np.float64) / 22050.0
    return (0.3 * np.sin(2.0 * np.pi * 220.0 * t) + 0.05 * rng.standard_normal(length)).astype(np.float32)


def bias_spectrum(seed: int = 11) -> np.ndarray:
    """2 |N(0, 1)| per bin, fp32"""
    return (2.0 * np.abs(np.random.default_rng(seed).standard_normal(BINS))).astype(np.float32)


def batch():
    """(audio fp32 [7, LD] with the signal in front and zeros behind, lengths)"""
    audio = np.zeros((len(LENGTHS), LD), dtype=np.float32)
    for b, n in enumerate(LENGTHS):
        audio[b, :n] = signal(n, 100 + b)
    return audio, np.asarray(LENGTHS, dtype=np.int32)


def hum(length: int) -> np.ndarray:
    """five fixed sinusoids, fp32: a stationary pattern like a generator's bias.  Cosines at bin centres: every frame, the reflected frame 0
    included, has the same magnitudes, so frame 0 as the bias at strength 1 removes all of it except behind the reflection at the far end
    (which breaks the pattern unless length - 1 is a multiple of 1024) -- a residue far above fp32 rounding, whose level can be compared"""
    i = np.arange(length, dtype=np.float64)
    parts = ((0.010, 46), (0.008, 100), (0.006, 153), (0.005, 256), (0.004, 371))
    return sum(a * np.cos(2.0 * np.pi * k * i / N) for a, k in parts).astype(np.float32)


def frame0_magnitude(x) -> np.ndarray:
    """sqrt(max(|DFT|^2, 1e-7)) of frame 0 in float64: what `STFTMagnitude(device, 1024, 256, 1024)(x)[0][0, 0]` measures (floor included)"""
    x = np.asarray(x, dtype=np.float64)
    return np.sqrt(np.maximum(np.abs(np.fft.rfft(window() * x[reflect(np.arange(N) - N // 2, x.shape[0])])) ** 2, 1e-7))


def level_db(x) -> float:
    return float(10.0 * np.log10(np.mean(np.asarray(x, dtype=np.float64) ** 2)))


_cache = {}


def reference_batch():
    """{strength: [out float64 per item]} and the share of clamped cells at strength 0.5 -- computed once per process"""
    if "ref" not in _cache:
        audio, lengths = batch()
        bias = bias_spectrum()
        ref, cells, clamped = {}, 0, 0
        for s in STRENGTHS:
            ref[s] = []
            for b, n in enumerate(lengths):
                st = {}
                ref[s].append(denoise(audio[b, :n], bias, s, st))
                if s == 0.5 and st:
                    cells, clamped = cells + st["cells"], clamped + st["clamped"]
        _cache["ref"] = (ref, clamped / cells)
    return _cache["ref"]


def yardstick():
    """max |fp32 torch.stft pipeline - float64 reference| over the batch's items and strengths (CPU), computed once per process"""
    if "yard" not in _cache:
        audio, lengths = batch()
        bias = bias_spectrum()
        import torch
        ref, _ = reference_batch()
        worst = 0.0
        for s in STRENGTHS:
            for b, n in enumerate(lengths):
                if n > N // 2:
                    worst = max(worst, float(np.abs(denoise_torch(audio[b, :n], bias, s, torch.float32) - ref[s][b]).max()))
        _cache["yard"] = worst
    return _cache["yard"]
