"""The definitions of the noise profile and the spectral gate (include/efts_abi.h, "Spectral gating of a corpus with a noise profile per
recording") in numpy float64: a plain loop over the frames, np.fft, sequential sums, no table.  Also the batch that the CPU and GPU tests
share, and the same two pipelines through torch.stft / torch.istft (float64: the check of this file; float32: the yardstick of the device's
error)."""
import numpy as np

N, H, BINS = 1024, 256, 513
LD = 12800
LENGTHS = (0, 512, 513, 1024, 4095, 4096, 4097, 12345)   # no frames, the copy path, T = 3, an unpaired last frame, both sides of a 16-hop run
EXTRA = ("zeros", "tone", "exact", "short")              # all zeros; a constant level; exactly MIN_FRAMES noise frames; MIN_FRAMES - 1
EXTRA_LEN = {"zeros": 4096, "tone": 4096, "exact": 8192, "short": 8192}
TOP_DB, MIN_FRAMES = 40.0, 8
STRENGTHS, FLOORS = (0.0, 1.0, 2.5), (0.0, 0.1, 1.0)
RATE = 22050.0


def ratio(top_db: float = TOP_DB) -> float:
    return float(10.0 ** (np.float64(top_db) / 10.0))


def window() -> np.ndarray:
    """periodic Hann, float64, rounded once to fp32 (what the device is given), as float64"""
    i = np.arange(N, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / N)).astype(np.float32).astype(np.float64)


def reflect(i: np.ndarray, length: int) -> np.ndarray:
    i = np.where(i < 0, -i, i)
    return np.where(i >= length, 2 * (length - 1) - i, i)


def frame_count(length: int) -> int:
    return 1 + length // H if length > N // 2 else 0


def seq_sum(v: np.ndarray) -> float:
    """v[0] + v[1] + .. in this order, float64"""
    return float(np.cumsum(np.asarray(v, dtype=np.float64))[-1]) if len(v) else 0.0


def frames_of(x: np.ndarray):
    """the item's frames [T, 1024] (fp32 samples, reflected) -- not yet windowed"""
    length = x.shape[0]
    T = frame_count(length)
    idx = reflect(H * np.arange(T)[:, None] - N // 2 + np.arange(N)[None, :], length) if T else np.zeros((0, N), dtype=np.int64)
    return x[idx]


def spectra(x: np.ndarray) -> np.ndarray:
    """X [T, 513] complex128: the DFT of the windowed frames, one np.fft.rfft per frame"""
    x = np.asarray(x, dtype=np.float64)
    fr = frames_of(x)
    return np.stack([np.fft.rfft(window() * f) for f in fr]) if fr.shape[0] else np.zeros((0, BINS), dtype=np.complex128)


def energies(x: np.ndarray) -> np.ndarray:
    """e[t] = sum_n (double) v^2, v = fl32(w[n] * x_t[n]): the one fp32 rounding of the definition is kept, the sum is sequential float64"""
    x = np.asarray(x, dtype=np.float32)
    w32 = window().astype(np.float32)
    return np.array([seq_sum((w32 * f).astype(np.float64) ** 2) for f in frames_of(x)], dtype=np.float64)


def noise_profile(x, top_db: float = TOP_DB, min_frames: int = MIN_FRAMES) -> dict:
    """x [len] fp32 -> profile float64 [513] (not rounded), noise_frames K, frames T, noise_db, flags [T] and margin_db: how far the nearest
    e[t] * r lies from e_max, in dB (inf without frames or for an all-zero item)"""
    x = np.asarray(x, dtype=np.float32)
    e = energies(x)
    T = e.shape[0]
    r = ratio(top_db)
    e_max = float(e.max()) if T else 0.0
    flags = e * r < e_max if T else np.zeros(0, dtype=bool)
    K = int(flags.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = float(np.abs(10.0 * np.log10(e * r / e_max)).min()) if T and e_max > 0 else float("inf")
    profile = np.zeros(BINS)
    if K >= max(min_frames, 1):
        m = np.abs(spectra(x))
        acc = np.zeros(BINS)
        for t in np.nonzero(flags)[0]:                    # ascending t; float64 addition of 8 to a few dozen terms: the grouping into runs
            acc = acc + m[t]                              # of 16 frames moves this by parts in 1e16, far below the fp32 rounding of the result
        profile = acc / K
    noise_db = float(10.0 * np.log10(seq_sum(e[flags]) / K / e_max)) if K else float("nan")
    return dict(profile=profile, noise_frames=K, frames=T, noise_db=noise_db, flags=flags, margin_db=margin, energies=e)


def gate(x, profile, strength: float, floor: float, bypass: bool = False) -> np.ndarray:
    """x [len] -> out [len], float64: tests/denoise_reference.py's loop with g = max(g, floor)"""
    x = np.asarray(x, dtype=np.float64)
    length = x.shape[0]
    T = frame_count(length)
    if T == 0 or bypass:
        return x.copy()
    w = window()
    sp = float(strength) * np.asarray(profile, dtype=np.float64)
    num, den = np.zeros(length + 2 * N), np.zeros(length + 2 * N)          # index s + 512
    for t in range(T):
        idx = reflect(H * t - N // 2 + np.arange(N), length)
        X = np.fft.rfft(w * x[idx])
        m = np.abs(X)
        d = m - sp
        g = np.where(d > 0, d / np.where(m > 0, m, 1.0), 0.0)
        g = np.maximum(g, float(floor))
        Y = g * X
        Y[0], Y[-1] = Y[0].real, Y[-1].real
        y = np.fft.irfft(Y, N)
        num[H * t:H * t + N] += w * y
        den[H * t:H * t + N] += w * w
    return (num / np.maximum(den, 1e-8))[N // 2:N // 2 + length]


def stft_torch(x, dtype):
    """X [513, T] through torch.stft on the CPU at `dtype`"""
    import torch
    xt = torch.as_tensor(np.asarray(x), dtype=dtype)
    w = torch.as_tensor(window(), dtype=dtype)
    return torch.stft(xt, N, H, N, window=w, center=True, pad_mode="reflect", return_complex=True), w


def profile_torch(x, flags, dtype) -> np.ndarray:
    """the mean magnitude over the flagged frames through torch.stft, mean at `dtype`"""
    import torch
    X, _ = stft_torch(x, dtype)
    return X.abs()[:, torch.as_tensor(np.asarray(flags))].mean(dim=1).numpy().astype(np.float64)


def gate_torch(x, profile, strength: float, floor: float, dtype) -> np.ndarray:
    """torch.stft -> gain -> torch.istft on the CPU at `dtype`"""
    import torch
    X, w = stft_torch(x, dtype)
    m = X.abs()
    d = m - torch.as_tensor(float(strength) * np.asarray(profile, dtype=np.float64), dtype=dtype)[:, None]
    g = torch.where(d > 0, d / torch.where(m > 0, m, torch.ones_like(m)), torch.zeros_like(m)).clamp(min=float(floor))
    return torch.istft(X * g, N, H, N, window=w, center=True, length=len(x)).numpy().astype(np.float64)


# ---- the batch
def quantise(x: np.ndarray) -> np.ndarray:
    return np.clip(np.round(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def coloured_noise(length: int, seed: int, rms: float) -> np.ndarray:
    """white noise through y[n] = 0.9 y[n - 1] + u[n], scaled to `rms`"""
    u = np.random.default_rng(seed).standard_normal(length + 64)
    y = np.zeros(length + 64)
    for n in range(1, length + 64):
        y[n] = 0.9 * y[n - 1] + u[n]
    y = y[64:]
    return y * (rms / max(float(np.sqrt(np.mean(y ** 2))), 1e-30)) if length else y


def harmonics(length: int) -> np.ndarray:
    """four harmonics of 220 Hz, peak 0.5"""
    t = np.arange(length, dtype=np.float64) / RATE
    v = sum(np.sin(2.0 * np.pi * 220.0 * k * t + 0.3 * k) / k for k in (1, 2, 3, 4))
    return 0.5 * v / max(float(np.abs(v).max()), 1e-30) if length else v


NOISE_RMS = 0.5 * 10.0 ** (-50.0 / 20.0)


def burst_item(length: int, seed: int) -> np.ndarray:
    """a harmonic burst of peak 0.5 in the middle third over stationary coloured noise 50 dB below it, int16"""
    x = coloured_noise(length, seed, NOISE_RMS)
    lo, hi = length // 3, (2 * length) // 3
    x[lo:hi] += harmonics(hi - lo)
    return quantise(x)


def tail_item(length: int, cut: int, seed: int) -> np.ndarray:
    """a 0.5-peak tone up to sample `cut`, the coloured noise alone behind it, int16"""
    x = coloured_noise(length, seed, NOISE_RMS)
    x[:cut] += harmonics(cut)
    return quantise(x)


_cache = {}


def batch():
    """(pcm int16 [12, LD], audio fp32 [12, LD] = fl32(pcm / 32768), lengths int32): the eight burst items, then EXTRA.  Zeros behind."""
    if "batch" not in _cache:
        items = [burst_item(n, 200 + b) for b, n in enumerate(LENGTHS)]
        n = EXTRA_LEN["exact"]
        T = frame_count(n)
        # frames t >= c + 2 lie wholly in the noise behind sample 256 c: K = T - c - 2
        items += [np.zeros(EXTRA_LEN["zeros"], np.int16), quantise(harmonics(EXTRA_LEN["tone"])),
                  tail_item(n, H * (T - 2 - MIN_FRAMES), 301), tail_item(n, H * (T - 1 - MIN_FRAMES), 302)]
        pcm = np.zeros((len(items), LD), dtype=np.int16)
        for b, v in enumerate(items):
            pcm[b, :v.shape[0]] = v
        lengths = np.asarray([v.shape[0] for v in items], dtype=np.int32)
        _cache["batch"] = (pcm, (pcm.astype(np.float32) / np.float32(32768.0)).astype(np.float32), lengths)
    return _cache["batch"]


def reference_profiles():
    """[noise_profile(item)] of the batch, computed once per process, after the condition on the inputs: every e[t] * r lies at least
    0.01 dB from e_max, so that the device's counts and flags must equal these"""
    if "prof" not in _cache:
        _, audio, lengths = batch()
        ref = [noise_profile(audio[b, :n]) for b, n in enumerate(lengths)]
        for b, p in enumerate(ref):
            assert p["margin_db"] >= 0.01, (b, p["margin_db"])
        _cache["prof"] = ref
    return _cache["prof"]


def profile_yardstick():
    """max |fp32 torch.stft mean - float64 reference| over the items with a profile (CPU), once per process"""
    if "pyard" not in _cache:
        import torch
        _, audio, lengths = batch()
        worst = 0.0
        for b, p in enumerate(reference_profiles()):
            if p["noise_frames"] >= MIN_FRAMES:
                worst = max(worst, float(np.abs(profile_torch(audio[b, :lengths[b]], p["flags"], torch.float32) - p["profile"]).max()))
        _cache["pyard"] = worst
    return _cache["pyard"]
