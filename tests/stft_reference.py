"""The definition of the STFT magnitudes and of the multi-resolution STFT distance (include/efts_abi.h), restated in numpy float64, and the
inputs that tests/test_stft_cpu.py and tests/test_stft_gpu.py share.  Only the window is fp32 (the definition rounds it once); everything
else -- samples, transform, magnitudes, sums -- is float64."""
import numpy as np

DEFAULT = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
CLAMP = 1e-7
MAX_WAV = 32768.0


def window(W):
    i = np.arange(W, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / W)).astype(np.float32)


def frame_count(L, N, H):
    return 1 + L // H if L > N // 2 else 0


def as_float64(x):
    """int16 PCM times 1 / max_wav_value, fp32 as it is"""
    x = np.asarray(x)
    return x.astype(np.float64) / MAX_WAV if x.dtype == np.int16 else x.astype(np.float64)


def magnitudes(x, N, H, W):
    """mag [T, N / 2 + 1] of one item (float64); T = 0 for an item of at most N / 2 samples"""
    x = as_float64(x)
    L = len(x)
    T = frame_count(L, N, H)
    if T == 0:
        return np.zeros((0, N // 2 + 1))
    padded = np.pad(x, N // 2, mode="reflect")
    w = np.zeros(N)
    off = (N - W) // 2
    w[off:off + W] = window(W).astype(np.float64)
    idx = H * np.arange(T)[:, None] + np.arange(N)[None, :]
    spec = np.fft.rfft(padded[idx] * w[None, :], axis=1)
    return np.sqrt(np.maximum(spec.real ** 2 + spec.imag ** 2, CLAMP))


def sums(x, y, N, H, W):
    """(num, den, l1, cells, share of cells at the clamp in either signal) of one item"""
    mx, my = magnitudes(x, N, H, W), magnitudes(y, N, H, W)
    floor = np.sqrt(CLAMP)
    share = float(np.mean((mx == floor) | (my == floor))) if mx.size else 0.0
    return float(((my - mx) ** 2).sum()), float((my ** 2).sum()), float(np.abs(np.log(my) - np.log(mx)).sum()), mx.size, share


def distance(x, y, lengths, resolutions=DEFAULT):
    """sc [B, R], log_mag [B, R], sums [B, R, 3], cells [B, R], clamped [B, R] of a padded batch"""
    B, R = len(lengths), len(resolutions)
    out = dict(sc=np.full((B, R), np.nan), log_mag=np.full((B, R), np.nan), sums=np.zeros((B, R, 3)), cells=np.zeros((B, R), dtype=np.int64),
               clamped=np.zeros((B, R)))
    for b, L in enumerate(lengths):
        for r, (N, H, W) in enumerate(resolutions):
            num, den, l1, cells, share = sums(x[b][:L], y[b][:L], N, H, W)
            out["sums"][b, r] = (num, den, l1)
            out["cells"][b, r] = cells
            out["clamped"][b, r] = share
            if cells:
                out["sc"][b, r] = np.sqrt(num) / np.sqrt(den)
                out["log_mag"][b, r] = l1 / cells
    return out


def batch_loss(out):
    """the reference's reduction of a batch: per resolution the Frobenius norms over all items and the mean over all cells, then the mean
    over the resolutions"""
    tot = out["sums"].sum(axis=0)
    return float(np.mean(np.sqrt(tot[:, 0]) / np.sqrt(tot[:, 1]))), float(np.mean(tot[:, 2] / out["cells"].sum(axis=0)))


# ---- the inputs of the distance tests: two sines plus noise, a stretch of exact zeros in the middle of BOTH signals, on the int16 grid
LENGTHS = (1025, 1024, 4099)


def zeros(L):
    return 1500 if L > 2048 else 0


def signal(L, seed):
    """(x fp32, y int16): y the 'recording', x a disturbed copy; both exactly 0 over ZEROS(L) samples in the middle of the item: long enough to
    hold whole frames of every default resolution in an item above 2048 samples (those cells sit at the clamp), too short for a whole frame of
    any of them in a shorter item (none does)"""
    rng = np.random.default_rng(seed)
    n = np.arange(L, dtype=np.float64)
    clean = 0.3 * np.sin(2 * np.pi * 220.0 / 22050.0 * n) + 0.2 * np.sin(2 * np.pi * 3100.0 / 22050.0 * n + 0.7)
    y = clean + 0.02 * rng.standard_normal(L)
    x = 0.9 * clean + 0.03 * rng.standard_normal(L)
    lo = (L - zeros(L)) // 2
    hi = lo + zeros(L)
    y[lo:hi] = 0.0
    x[lo:hi] = 0.0
    y16 = np.round(y * MAX_WAV).clip(-32768, 32767).astype(np.int16)
    x16 = np.round(x * MAX_WAV).clip(-32768, 32767).astype(np.int16)
    return (x16.astype(np.float32) / np.float32(MAX_WAV)).astype(np.float32), y16


def batch(lengths=LENGTHS, seed=0, fill=None):
    """x fp32 [B, max], y int16 [B, max]; behind an item's length zeros, or with `fill` = a seed, garbage"""
    n = max(lengths)
    x = np.zeros((len(lengths), n), dtype=np.float32)
    y = np.zeros((len(lengths), n), dtype=np.int16)
    if fill is not None:
        rng = np.random.default_rng(fill)
        x[:] = rng.uniform(-1, 1, x.shape).astype(np.float32)
        y[:] = rng.integers(-32768, 32767, y.shape)
    for b, L in enumerate(lengths):
        x[b, :L], y[b, :L] = signal(L, seed + b)
    return x, y


# ---- the inputs of tests/test_audio_boundaries_*.py: items whose frames end on either side of what one workgroup of stft_kernel takes
# (2 UPB frames) and of what one step of stft_reduce_kernel sums (ST_CHUNK frames)
FRAMES_PER_WORKGROUP = {256: 256, 512: 128, 1024: 64, 2048: 32}      # 2 * st_cfg<N>::UPB (csrc/efts_stft.hip:40)
REDUCE_CHUNK = 1024                                                   # ST_CHUNK (csrc/efts_stft.hip:27)
BOUNDARY_MAG = ((256, 64, 256), (512, 50, 240), (1024, 120, 600))     # the smallest hop the project uses at each size
BOUNDARY_DIST = (512, 50, 240)
BOUNDARY_DIST_FRAMES = (1024, 1025, 2049, 130)


def boundary_mag_lengths(N, H):
    """T = 2 UPB - 1, 2 UPB, 2 UPB + 1, 2 UPB + 2: the first workgroup ends on an unpaired frame, is exactly full, then the second one holds
    an unpaired frame, then one pair"""
    per = FRAMES_PER_WORKGROUP[N]
    return tuple(H * (T - 1) for T in (per - 1, per, per + 1, per + 2))


def boundary_dist_lengths():
    return tuple(BOUNDARY_DIST[1] * (T - 1) for T in BOUNDARY_DIST_FRAMES)


def boundary_batch(lengths, seed, fp32_x=True):
    """x (fp32 with NaN behind every item, or int16 with -32768 there) and y (int16, -32768 behind every item) of signal()"""
    n = max(lengths)
    x = np.full((len(lengths), n), np.nan, dtype=np.float32) if fp32_x else np.full((len(lengths), n), -32768, dtype=np.int16)
    y = np.full((len(lengths), n), -32768, dtype=np.int16)
    for b, L in enumerate(lengths):
        xf, y[b, :L] = signal(L, seed + b)
        x[b, :L] = xf if fp32_x else np.round(xf * np.float32(MAX_WAV)).astype(np.int16)
    return x, y
