"""numpy restatement of the true-peak and peak-limiter definition (include/efts_abi.h, "True-peak metering after ITU-R BS.1770 Annex 2") with
direct sums, and the inputs that tests/test_limiter_cpu.py and tests/test_limiter_gpu.py share.  Never imports the product.  Every function
takes the dtype it computes in: float64 is the reference, float32 -- every array and every sum in fp32 numpy, a product and a sum rounding
separately -- is the yardstick for the device's error."""
import functools
import math

import numpy as np

PHASES, ZEROS, BETA = 4, 12, 8.0
TAPS = 2 * ZEROS + 1
CHUNK = 2048                                   # EFTS_LIMITER_CHUNK (tests/test_limiter_cpu.py compares it with the header)
MAX_HOLD = 128
RATE = 22050
LENGTHS = (0, 1, 12, 13, CHUNK - 1, CHUNK, CHUNK + 1, 12345)         # of the click signal; three more items follow them
UNDER, ZERO, SINE = 8, 9, 10                   # their rows: wholly under both ceilings, all zero, the fs / 4 sine
EXTRA_LENGTHS = (3000, 3000, 4099)
N = 12352                                      # samples per row of the batch
CEILINGS = (0.5, float(np.float32(10.0 ** (-1.0 / 20.0))))           # as the fp32 values that the kernel compares with
HOLD_SMOOTH = ((32, 32), (64, 32), (16, 8), (128, 1))
SEED = 0                                       # chosen so that the condition of tests/test_limiter_cpu.py holds: no case was dropped for it


def bessel_i0(v: float) -> float:
    """the series sum of ((v / 2)^k / k!)^2, until a term no longer changes the sum"""
    total, term, k = 1.0, 1.0, 0
    while True:
        k += 1
        term *= (v / 2.0) / k
        if total + term * term == total:
            return total
        total += term * term


@functools.lru_cache(maxsize=None)
def table64() -> np.ndarray:
    """float64 [4, 25] before the one rounding to fp32, entry by entry from the formula"""
    h = np.zeros((PHASES, TAPS))
    for q in range(PHASES):
        for k in range(-ZEROS, ZEROS + 1):
            t = q / PHASES - k
            if abs(t) >= ZEROS:
                continue
            sinc = (1.0 if t == 0 else 0.0) if t == int(t) else math.sin(math.pi * t) / (math.pi * t)
            h[q, k + ZEROS] = sinc * bessel_i0(BETA * math.sqrt(1.0 - (t / ZEROS) ** 2)) / bessel_i0(BETA)
    return h


def table32() -> np.ndarray:
    return table64().astype(np.float32)


def samples(x: np.ndarray, dtype, max_wav_value: float = 32768.0) -> np.ndarray:
    """the item's samples as the definition takes them: int16 as x / max_wav_value"""
    if x.dtype == np.int16:
        return (x.astype(np.float32) * np.float32(1.0 / max_wav_value)).astype(dtype)
    return x.astype(dtype)


def oversampled_peak(x: np.ndarray, dtype) -> np.ndarray:
    """p[i], i = 0 .. len - 1, of samples x (already `samples`): k ascending, zeros outside the item"""
    n = x.shape[0]
    h = table32().astype(dtype)
    xp = np.concatenate([np.zeros(ZEROS, dtype), x.astype(dtype), np.zeros(ZEROS, dtype)])
    p = np.abs(x.astype(dtype))
    for q in range(1, PHASES):
        acc = np.zeros(n, dtype)
        for k in range(-ZEROS, ZEROS + 1):
            acc = acc + xp[ZEROS + k:ZEROS + k + n] * h[q, k + ZEROS]
        p = np.maximum(p, np.abs(acc))
    return p


def peaks(x: np.ndarray, dtype):
    """(true peak, sample peak) of one item, 0 for an empty one"""
    x = samples(x, dtype)
    if x.shape[0] == 0:
        return dtype(0.0), dtype(0.0)
    return oversampled_peak(x, dtype).max(), np.abs(x).max()


def limit(x: np.ndarray, ceiling: float, hold: int, smooth: int, dtype) -> dict:
    """the limiter on one item: out, the curves p, r, m (on -smooth .. len + smooth - 1), g and the three statistics"""
    assert 1 <= smooth <= hold <= MAX_HOLD
    x = samples(x, dtype)
    n = x.shape[0]
    c = dtype(ceiling)
    p = oversampled_peak(x, dtype)
    over = p > c
    r = np.where(over, c / np.where(over, p, dtype(1.0)), dtype(1.0)).astype(dtype)
    rp = np.concatenate([np.ones(hold + smooth, dtype), r, np.ones(hold + smooth, dtype)])
    m = np.ones(n + 2 * smooth, dtype)
    for j in range(2 * hold + 1):
        m = np.minimum(m, rp[j:j + n + 2 * smooth])
    s = np.zeros(n, dtype)
    for e in range(2 * smooth + 1):
        s = s + m[e:e + n]
    g = np.minimum(r, s / dtype(2 * smooth + 1))
    return dict(out=x * g, p=p, r=r, m=m, g=g, gain_min=g.min() if n else dtype(1.0), limited=int((g < 1).sum()),
                true_peak_in=p.max() if n else dtype(0.0))


def click_signal(n: int, seed: int) -> np.ndarray:
    """a 220 Hz tone modulated at 3 Hz plus a 3 kHz tone plus noise, with +0.9 and -0.9 on the two samples in its middle"""
    t = np.arange(n, dtype=np.float64) / RATE
    rng = np.random.default_rng(seed)
    x = 0.35 * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t + 1.0)) * np.sin(2 * np.pi * 220.0 * t) + 0.1 * np.sin(2 * np.pi * 3000.0 * t + 0.3)
    x = x + 0.02 * rng.uniform(-1.0, 1.0, size=n)
    if n:
        x[n // 2] = 0.9
    if n // 2 + 1 < n:
        x[n // 2 + 1] = -0.9
    return x


def fs4_sine(n: int) -> np.ndarray:
    """amplitude 1 at fs / 4 with 45 degrees of phase: every sample is +-0.7071, the signal between them reaches 1"""
    return np.sin(2 * np.pi * 0.25 * np.arange(n, dtype=np.float64) + np.pi / 4)


@functools.lru_cache(maxsize=None)
def batch(pcm16: bool = False):
    """(audio [11, N], lengths): full scale behind every length"""
    lengths = np.asarray(LENGTHS + EXTRA_LENGTHS, dtype=np.int64)
    rows = [click_signal(n, SEED + 10 * b) for b, n in enumerate(LENGTHS)]
    t = np.arange(EXTRA_LENGTHS[0], dtype=np.float64) / RATE
    rows.append(0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.1 * np.sin(2 * np.pi * 5000.0 * t + 0.5))
    rows.append(np.zeros(EXTRA_LENGTHS[1]))
    rows.append(fs4_sine(EXTRA_LENGTHS[2]))
    audio = np.ones((len(rows), N), np.float64)
    for b, row in enumerate(rows):
        audio[b, :row.shape[0]] = row
    if pcm16:
        audio = np.round(audio * 32767.0).astype(np.int16)
    else:
        audio = audio.astype(np.float32)
    audio.setflags(write=False)
    lengths.setflags(write=False)
    return audio, lengths


def items(pcm16: bool = False):
    audio, lengths = batch(pcm16)
    return [audio[b, :int(n)] for b, n in enumerate(lengths)]


@functools.lru_cache(maxsize=None)
def peaks_batch(pcm16: bool, dtype_name: str):
    dtype = np.dtype(dtype_name).type
    return [peaks(x, dtype) for x in items(pcm16)]


@functools.lru_cache(maxsize=None)
def limit_batch(pcm16: bool, ceiling: float, hold: int, smooth: int, dtype_name: str):
    """`limit` of every item of the batch, and the (true peak, sample peak) of every output"""
    dtype = np.dtype(dtype_name).type
    res = [limit(x, ceiling, hold, smooth, dtype) for x in items(pcm16)]
    for r in res:
        r["true_peak_out"] = peaks(r["out"], dtype)[0]
    return res


def cases():
    return [(pcm16, c, h, s) for pcm16 in (False, True) for c in CEILINGS for h, s in HOLD_SMOOTH]


def excess_db(true_peak: float, ceiling: float) -> float:
    return 20.0 * math.log10(true_peak / ceiling) if true_peak > 0 else float("-inf")
