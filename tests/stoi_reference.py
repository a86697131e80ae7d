"""The definition of STOI and ESTOI (include/efts_abi.h, "Short-time objective intelligibility") in numpy: plain loops over frames and
segments and np.fft, in float64 -- the reference -- or, with dtype=np.float32, the same definition with every array and every sum in fp32: the
yardstick for the device's error.  Also the inputs that the CPU and GPU tests share."""
import numpy as np

FS, FRAME, HOP, N_FFT, BANDS, SEGMENT, BETA, DYN_RANGE = 10000, 256, 128, 512, 15, 30, -15.0, 40.0
BAND_TABLE = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138),
              (138, 174), (174, 219))


def window() -> np.ndarray:
    """w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), float64, rounded once to fp32 (what the device is given), as float64"""
    i = np.arange(FRAME, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 1.0) / (FRAME + 1.0))).astype(np.float32).astype(np.float64)


def bands_from_formula():
    """[lo, hi) per band: the bins nearest to 150 * 2^((2 j -+ 1) / 6) Hz on the grid f * 10000 / 512, as the reference code's thirdoct finds them"""
    grid = np.linspace(0, FS, N_FFT + 1)[:N_FFT // 2 + 1]
    out = []
    for j in range(BANDS):
        lo, hi = 150.0 * 2.0 ** ((2 * j - 1) / 6.0), 150.0 * 2.0 ** ((2 * j + 1) / 6.0)
        out.append((int(np.argmin((grid - lo) ** 2)), int(np.argmin((grid - hi) ** 2))))
    return tuple(out)


def frame_count(n: int) -> int:
    return (n - FRAME) // HOP + 1 if n >= FRAME else 0


def _normalise(a, axis, eps):
    a = a - a.mean(axis=axis, keepdims=True)
    return a / (np.sqrt((a * a).sum(axis=axis, keepdims=True)) + eps)


def stoi(x, y, dtype=np.float64) -> dict:
    """x, y [n] -> dict(stoi, estoi, frames, kept, segments, margin_db): the two scores (nan without a segment), F, K, M and the smallest
    distance of any frame's energy from the 40 dB threshold in dB (inf for no frames or an all-zero x)"""
    dt = np.dtype(dtype)
    x, y = np.asarray(x).astype(dt), np.asarray(y).astype(dt)
    n = min(x.shape[0], y.shape[0])
    w = window().astype(dt)
    F = frame_count(n)
    out = dict(stoi=float("nan"), estoi=float("nan"), frames=F, kept=0, segments=0, margin_db=float("inf"))
    if F == 0:
        return out
    idx = HOP * np.arange(F)[:, None] + np.arange(FRAME)[None, :]
    xf, yf = w * x[idx], w * y[idx]                                    # [F, 256]
    e = (xf * xf).sum(axis=1)
    e_max = e.max()
    if not e_max > 0:
        return out
    keep = e.astype(np.float64) * 1e4 > np.float64(e_max)
    with np.errstate(divide="ignore"):
        out["margin_db"] = float(np.abs(10.0 * np.log10(e.astype(np.float64) * 1e4 / np.float64(e_max))).min())
    K = int(keep.sum())
    out["kept"] = K
    if K <= SEGMENT:
        return out
    xs, ys = np.zeros(HOP * (K - 1) + FRAME, dt), np.zeros(HOP * (K - 1) + FRAME, dt)
    for j, k in enumerate(np.nonzero(keep)[0]):                         # ascending j: the older frame first
        xs[HOP * j:HOP * j + FRAME] += xf[k]
        ys[HOP * j:HOP * j + FRAME] += yf[k]
    T = K - 1
    idx = HOP * np.arange(T)[:, None] + np.arange(FRAME)[None, :]
    PX = np.abs(np.fft.rfft(w * xs[idx], N_FFT, axis=1)) ** 2            # [T, 257]; numpy's rfft keeps fp32 for fp32 input
    PY = np.abs(np.fft.rfft(w * ys[idx], N_FFT, axis=1)) ** 2
    assert PX.dtype == dt
    X = np.stack([np.sqrt(PX[:, lo:hi].sum(axis=1)) for lo, hi in BAND_TABLE], axis=0)      # [15, T]
    Y = np.stack([np.sqrt(PY[:, lo:hi].sum(axis=1)) for lo, hi in BAND_TABLE], axis=0)
    M = T - (SEGMENT - 1)
    eps = dt.type(np.finfo(np.float64).eps)
    clip = dt.type(1.0 + 10.0 ** (-BETA / 20.0))
    d_sum, e_sum = dt.type(0), dt.type(0)
    for m in range(M):
        xb, yb = X[:, m:m + SEGMENT], Y[:, m:m + SEGMENT]              # [15, 30]
        c = np.sqrt((xb * xb).sum(axis=1, keepdims=True)) / (np.sqrt((yb * yb).sum(axis=1, keepdims=True)) + eps)
        yp = np.minimum(c * yb, xb * clip)
        d_sum += (_normalise(xb, 1, eps) * _normalise(yp, 1, eps)).sum()
        xn, yn = _normalise(_normalise(xb, 1, eps), 0, eps), _normalise(_normalise(yb, 1, eps), 0, eps)
        e_sum += (xn * yn).sum()
    assert np.asarray(d_sum).dtype == dt
    out.update(stoi=float(d_sum / dt.type(BANDS * M)), estoi=float(e_sum / dt.type(SEGMENT * M)), segments=M)
    return out


# ---- the inputs of the tests

def speech_like(n: int, seed: int) -> np.ndarray:
    """24 harmonics, amplitude 0.1 each, of a fundamental that moves slowly between 80 and 160 Hz, under a max(sin, 0)^2 syllable envelope at
    about 1.1 Hz, on a noise floor of 1e-4; fp32 at 10 000 Hz.  About half of its frames are silent by the 40 dB rule."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / FS
    f0 = 120.0 + 40.0 * np.sin(2.0 * np.pi * 0.37 * t + rng.uniform(0, 2 * np.pi))
    phase = 2.0 * np.pi * np.cumsum(f0) / FS
    voice = sum(0.1 * np.sin(h * phase + rng.uniform(0, 2 * np.pi)) for h in range(1, 25))
    env = np.maximum(np.sin(2.0 * np.pi * 1.1 * t + rng.uniform(0, 2 * np.pi)), 0.0) ** 2
    return (env * voice + 1e-4 * rng.standard_normal(n)).astype(np.float32)


def add_noise(x: np.ndarray, snr_db: float, seed: int) -> np.ndarray:
    """x + white noise at `snr_db` against x's mean power, fp32"""
    rng = np.random.default_rng(seed)
    p = float(np.mean(np.asarray(x, dtype=np.float64) ** 2))
    return (x + np.sqrt(p / 10.0 ** (snr_db / 10.0)) * rng.standard_normal(x.shape[0])).astype(np.float32)


def truncate_to_kept(x: np.ndarray, K: int) -> int:
    """the smallest n for which the reference keeps K frames of x[:n]"""
    for n in range(FRAME, x.shape[0] + 1, HOP):
        if stoi(x[:n], x[:n])["kept"] >= K:
            assert stoi(x[:n], x[:n])["kept"] == K
            return n
    raise AssertionError(f"x never keeps {K} frames")


LD = 23456
SNRS = (None, 20.0, 5.0, -5.0)           # y = x itself, then x plus noise

_cache = {}


def batch():
    """(x fp32 [6, LD], lengths, names): n = 255; an item truncated to K = 30; one to K = 31; about 15 000 and 23 456 samples; an all-zero x.
    Zeros behind every item."""
    if "batch" not in _cache:
        base = speech_like(LD, 7)
        n30, n31 = truncate_to_kept(base, 30), truncate_to_kept(base, 31)
        lengths = [255, n30, n31, 15001, LD, 12000]
        x = np.zeros((len(lengths), LD), dtype=np.float32)
        x[0, :255] = base[:255]
        x[1, :n30] = base[:n30]
        x[2, :n31] = base[:n31]
        x[3, :15001] = speech_like(15001, 8)
        x[4] = speech_like(LD, 9)
        _cache["batch"] = (x, np.asarray(lengths, dtype=np.int32), ("n255", "K30", "K31", "15001", "23456", "zero_x"))
    return _cache["batch"]


def processed(snr):
    """y [6, LD] for one entry of SNRS; the all-zero item's y is noise alone"""
    key = ("y", snr)
    if key not in _cache:
        x, lengths, _ = batch()
        y = x.copy()
        if snr is not None:
            for b, n in enumerate(lengths):
                y[b, :n] = add_noise(x[b, :n], snr, 1000 + b) if x[b, :n].any() else (0.01 * np.random.default_rng(b).standard_normal(n)).astype(np.float32)
        _cache[key] = y
    return _cache[key]


def to_pcm16(a: np.ndarray) -> np.ndarray:
    return np.clip(np.round(a.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def reference_batch(pcm16: bool = False, dtype=np.float64):
    """{snr: [stoi() dict per item]} on the batch (through int16 and back when `pcm16`) -- computed once per process, never changed"""
    key = ("ref", pcm16, np.dtype(dtype).name)
    if key not in _cache:
        x, lengths, _ = batch()
        conv = (lambda a: to_pcm16(a).astype(np.float32) * np.float32(1.0 / 32768.0)) if pcm16 else (lambda a: a)
        _cache[key] = {snr: [stoi(conv(x[b, :n]), conv(processed(snr)[b, :n]), dtype) for b, n in enumerate(lengths)] for snr in SNRS}
    return _cache[key]


def yardstick(pcm16: bool = False) -> float:
    """max |fp32 definition - float64 reference| over both scores of every scored item of the batch (CPU)"""
    ref, low = reference_batch(pcm16), reference_batch(pcm16, np.float32)
    worst = 0.0
    for snr in SNRS:
        for r, q in zip(ref[snr], low[snr]):
            assert (r["frames"], r["kept"], r["segments"]) == (q["frames"], q["kept"], q["segments"])
            if r["segments"]:
                worst = max(worst, abs(q["stoi"] - r["stoi"]), abs(q["estoi"] - r["estoi"]))
    return worst


# ---- the inputs of tests/test_audio_boundaries_*.py: items long enough to leave the first turn of stoi_select_kernel's scan (256 frames)
# and the first chunk of stoi_reduce_kernel's sum (512 segments)

def frame_energies(x) -> np.ndarray:
    """e[f] of stoi(): the float64 energies of the windowed frames of x"""
    x = np.asarray(x).astype(np.float64)
    F = frame_count(x.shape[0])
    idx = HOP * np.arange(F)[:, None] + np.arange(FRAME)[None, :]
    xf = window() * x[idx]
    return (xf * xf).sum(axis=1)


def keep_flags(x) -> np.ndarray:
    """the frames stoi() keeps: e 10^4 > e_max"""
    e = frame_energies(x)
    return e * 1e4 > e.max() if e.size else np.zeros(0, dtype=bool)


def truncate_to_kept_fast(x: np.ndarray, K: int) -> int:
    """truncate_to_kept(x, K) from the frame energies alone: a prefix of F' frames keeps the frames whose energy times 10^4 exceeds the
    running maximum over that prefix"""
    e = frame_energies(x)
    for F in range(1, e.shape[0] + 1):
        kept = int((e[:F] * 1e4 > e[:F].max()).sum())
        if kept >= K:
            assert kept == K
            return FRAME + HOP * (F - 1)
    raise AssertionError(f"x never keeps {K} frames")


def dense(n: int, seed: int) -> np.ndarray:
    """a stationary complex of 12 tones between 200 and 3500 Hz, amplitude 0.05 each, plus white noise of 0.01: no frame is silent by the 40 dB
    rule; fp32 at 10 000 Hz"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / FS
    tones = sum(0.05 * np.sin(2.0 * np.pi * f * t + rng.uniform(0, 2 * np.pi)) for f in np.linspace(200.0, 3500.0, 12))
    return (tones + 0.01 * rng.standard_normal(n)).astype(np.float32)


def add_ramped_noise(x: np.ndarray, snr_from: float, snr_to: float, seed: int) -> np.ndarray:
    """x + white noise whose level moves linearly in dB from `snr_from` to `snr_to` against x's mean power over the item: the segments' sums
    then differ along the item, so a sum that takes the wrong segments is a wrong sum.  fp32"""
    rng = np.random.default_rng(seed)
    p = float(np.mean(np.asarray(x, dtype=np.float64) ** 2))
    snr = np.linspace(snr_from, snr_to, x.shape[0])
    return (x + np.sqrt(p / 10.0 ** (snr / 10.0)) * rng.standard_normal(x.shape[0])).astype(np.float32)


def length_of_frames(F: int) -> int:
    return FRAME + HOP * (F - 1)


SCAN_FRAMES = (256, 257, 300, 182)            # the last one is the neighbour that ends inside the first turn
SCAN_SEEDS = (34, 33, 35, 36)                 # searched: tests/test_audio_boundaries_cpu.py checks what they must give
REDUCE_SEGMENTS = (512, 513, 1025, 513, 60)   # M per item; the fourth is speech_like truncated to K = 543, the last the short neighbour
REDUCE_SEEDS = (41, 42, 43, 46, 45)


def boundary_batch(which: str):
    """(x fp32 [B, ld], y fp32 [B, ld], lengths, names) with NaN behind every item.
    "scan": speech_like items of 256, 257 and 300 frames and one of 182.
    "reduce": dense items with M = 512, 513 and 1025 segments, one speech_like item truncated to K = 543 kept frames, one speech_like
    item of about 60 segments."""
    key = ("boundary", which)
    if key not in _cache:
        items = []
        if which == "scan":
            for F, seed in zip(SCAN_FRAMES, SCAN_SEEDS):
                items.append((f"F{F}", speech_like(length_of_frames(F), seed)))
        else:
            for i, (M, seed) in enumerate(zip(REDUCE_SEGMENTS, REDUCE_SEEDS)):
                if i < 3:
                    items.append((f"dense_M{M}", dense(length_of_frames(M + SEGMENT), seed)))
                elif i == 3:
                    full = speech_like(160000, seed)
                    items.append((f"speech_K{M + SEGMENT}", full[:truncate_to_kept_fast(full, M + SEGMENT)]))
                else:
                    items.append(("speech_short", speech_like(LD, seed)))
        lengths = np.asarray([len(v) for _, v in items], dtype=np.int32)
        x = np.full((len(items), int(lengths.max())), np.nan, dtype=np.float32)
        y = x.copy()
        for b, (_, v) in enumerate(items):
            x[b, :len(v)] = v
            y[b, :len(v)] = add_ramped_noise(v, 15.0, -5.0, 2000 + b)
        for v in (x, y, lengths):
            v.setflags(write=False)
        _cache[key] = (x, y, lengths, tuple(name for name, _ in items))
    return _cache[key]


def boundary_pcm16(a: np.ndarray, lengths) -> np.ndarray:
    """the batch as int16, -32768 behind every item"""
    out = np.full(a.shape, -32768, dtype=np.int16)
    for b, n in enumerate(lengths):
        out[b, :n] = to_pcm16(a[b, :n])
    return out


def boundary_reference(which: str, pcm16: bool = False, dtype=np.float64):
    """[stoi() dict per item] of boundary_batch(which) (through int16 and back when `pcm16`) -- computed once per process"""
    key = ("boundary_ref", which, pcm16, np.dtype(dtype).name)
    if key not in _cache:
        x, y, lengths, _ = boundary_batch(which)
        conv = (lambda a: to_pcm16(a).astype(np.float32) * np.float32(1.0 / 32768.0)) if pcm16 else (lambda a: a)
        _cache[key] = [stoi(conv(x[b, :n]), conv(y[b, :n]), dtype) for b, n in enumerate(lengths)]
    return _cache[key]


def boundary_yardstick(which: str, pcm16: bool = False) -> float:
    """max |fp32 definition - float64 reference| over both scores of every item of boundary_batch(which) (CPU)"""
    worst = 0.0
    for r, q in zip(boundary_reference(which, pcm16), boundary_reference(which, pcm16, np.float32)):
        assert (r["frames"], r["kept"], r["segments"]) == (q["frames"], q["kept"], q["segments"])
        if r["segments"]:
            worst = max(worst, abs(q["stoi"] - r["stoi"]), abs(q["estoi"] - r["estoi"]))
    return worst
