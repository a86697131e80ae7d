"""numpy float64 restatement of the loudness definition (include/efts_abi.h, "Integrated loudness after ITU-R BS.1770"), and the inputs that
the CPU and GPU tests share.  It never sees the product's code.

The K-weighting filter here is STRICTLY SEQUENTIAL over the whole item (scipy.signal.lfilter, float64): what the device's segmented
filter with its 0.2 s warm-up is measured against.  `margin_lu` says how far the nearest block power lies from either gate, in LU: the
condition under which the gate decisions of two correct implementations must agree.
"""
import math

import numpy as np
from scipy.signal import lfilter

GAMMA_A = 10.0 ** ((-70.0 + 0.691) / 10.0)
SEGMENT = 512                                                          # EFTS_LOUDNESS_SEGMENT, pinned by tests/test_loudness_cpu.py


def coefficients(fs):
    """(b_shelf, a_shelf, b_high, a_high), float64: the bilinear designs of libebur128"""
    K = math.tan(math.pi * 1681.974450955533 / fs)
    Q = 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    bs = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    as_ = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    K = math.tan(math.pi * 38.13547087602444 / fs)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    return bs, as_, np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])


def _down(v):
    """the largest float32 <= the float64 v (v > 0)"""
    f = np.float32(v)
    return f if np.float64(f) <= v else np.nextafter(f, np.float32(0.0))


def measure(x, fs, target=-23.0, ceiling=None, max_wav_value=32768.0):
    """x: one item, int16 or float32 [len].  Returns dict(lufs, gain float32, flags, blocks (|A|, |G|), z, margin_lu, ceiling_margin)."""
    x = np.asarray(x)
    pcm = x.dtype == np.int16
    assert pcm or x.dtype == np.float32
    assert 8000 <= fs <= 48000 and fs % 10 == 0
    scale = np.float64(np.float32(1.0 / max_wav_value)) if pcm else np.float64(1.0)
    xs = x.astype(np.float64) * scale
    bs, as_, bh, ah = coefficients(fs)
    y = lfilter(bh, ah, lfilter(bs, as_, xs)) if xs.size else xs
    h = fs // 10
    nb = xs.size // h
    sub = (y[:nb * h] ** 2).reshape(nb, h).sum(axis=1)
    z = np.array([sub[j:j + 4].sum() / (4.0 * h) for j in range(max(nb - 3, 0))], dtype=np.float64)
    margin = np.inf
    A = z[z > GAMMA_A]
    lufs, flags, G = -np.inf, 0, A[:0]
    if z.size:
        margin = min(margin, float(np.abs(10.0 * np.log10(np.maximum(z, 1e-300) / GAMMA_A)).min()))
    if A.size:
        gamma_r = 0.1 * A.mean()
        margin = min(margin, float(np.abs(10.0 * np.log10(A / gamma_r)).min()))
        G = A[A > gamma_r]
        lufs = -0.691 + 10.0 * np.log10(G.mean())
    else:
        flags |= 1
    raw_peak = np.float32(np.abs(x.astype(np.float64)).max()) if x.size else np.float32(0.0)     # int16: |raw| <= 32768, exact in float32
    gain, ceiling_margin = np.float32(scale), np.inf
    if not flags & 1:
        g = 10.0 ** ((target - lufs) / 20.0)
        p = np.float64(raw_peak) * scale
        if ceiling is not None:
            ceiling_margin = abs(g * p / ceiling - 1.0)
        if ceiling is not None and g * p > ceiling:
            flags |= 2
            gain = _down((ceiling / p) * scale)
            while np.float64(np.float32(raw_peak * gain)) > ceiling:
                gain = np.nextafter(gain, np.float32(0.0))
        else:
            gain = np.float32(g * scale)
    return dict(lufs=float(lufs), gain=np.float32(gain), flags=flags, blocks=(int(A.size), int(G.size)), z=z, margin_lu=margin,
                ceiling_margin=ceiling_margin)


# ---------------------------------------------------------------------------------------------------------------- the shared inputs
def _quantise(x):
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)


def _bursts(rng, n, fs, loud=0.3, quiet_db=-50.0):
    """uniform noise: 0.5 s loud, 0.5 s `quiet_db` under it, and so on"""
    amp = np.where((np.arange(n) // (fs // 2)) % 2 == 0, loud, loud * 10.0 ** (quiet_db / 20.0))
    return rng.uniform(-1.0, 1.0, size=n) * amp


def _tone(n, fs, f, a):
    return a * np.sin(2.0 * np.pi * f * np.arange(n) / fs)


def cases():
    """name -> dict(fs, x int16 [B, n], lengths, target, ceiling).  The padding behind every length is full scale, and the row of length 0
    is loud throughout: nothing behind a length may be read.  The fp32 twin of a case is `as_float(x)`: the same integers times 2^-15."""
    rng = np.random.default_rng(1770)
    out = {}
    # the main case: 3 s at 22 050 Hz; bursts (the relative gate drops blocks), noise on a tone, one sample short of four sub-blocks, nothing
    fs, n = 22050, 66150
    lengths = [66150, 40000, 8819, 0]
    x = np.full((4, n), 32767, dtype=np.int16)
    x[0, :lengths[0]] = _quantise(_bursts(rng, lengths[0], fs))
    x[1, :lengths[1]] = _quantise(_tone(lengths[1], fs, 440.0, 0.2) + rng.uniform(-0.05, 0.05, size=lengths[1]))
    x[2, :lengths[2]] = _quantise(rng.uniform(-0.5, 0.5, size=lengths[2]))
    out["main"] = dict(fs=fs, x=x, lengths=lengths, target=-23.0, ceiling=0.99)
    # 48 kHz, 2 s: the slowest decay counted in samples
    fs, n = 48000, 96000
    lengths = [96000, 70001]
    x = np.full((2, n), -32768, dtype=np.int16)
    x[0] = _quantise(_bursts(rng, n, fs, loud=0.2, quiet_db=-30.0) + 0.05)
    x[1, :lengths[1]] = _quantise(_tone(lengths[1], fs, 997.0, 0.25) + rng.uniform(-0.01, 0.01, size=lengths[1]))
    out["48k"] = dict(fs=fs, x=x, lengths=lengths, target=-27.0, ceiling=0.99)
    # a DC offset plus a 30 Hz tone (under the high-pass corner) and a little noise: the worst case for what the high-pass holds
    fs, n = 22050, 44100
    lengths = [44100, 30000]
    x = np.full((2, n), 32767, dtype=np.int16)
    for b, v in enumerate(lengths):
        x[b, :v] = _quantise(0.4 + _tone(v, fs, 30.0, 0.3) + rng.uniform(-0.02, 0.02, size=v))
    out["dc"] = dict(fs=fs, x=x, lengths=lengths, target=-23.0, ceiling=None)
    # lengths one below, at and one above a multiple of the segment (512 * 20) and of h (2205 * 5)
    fs = 22050
    lengths = [10239, 10240, 10241, 11024, 11025, 11026]
    x = np.full((6, 11026), 32767, dtype=np.int16)
    for b, v in enumerate(lengths):
        x[b, :v] = _quantise(_tone(v, fs, 200.0 + 50.0 * b, 0.1) + rng.uniform(-0.1, 0.1, size=v))
    out["edges"] = dict(fs=fs, x=x, lengths=lengths, target=-23.0, ceiling=0.99)
    # the ceiling limits: clicks of full scale on quiet noise, and a loud target
    fs, n = 16000, 16000
    lengths = [16000, 12000]
    x = np.full((2, n), 32767, dtype=np.int16)
    for b, v in enumerate(lengths):
        s = rng.uniform(-0.02, 0.02, size=v)
        s[::1000] = 0.9
        x[b, :v] = _quantise(s)
    out["ceiling"] = dict(fs=fs, x=x, lengths=lengths, target=-14.0, ceiling=0.5)
    for c in out.values():
        c["x"].setflags(write=False)
    return out


def as_float(x):
    return (x.astype(np.float32) * np.float32(2.0 ** -15)).astype(np.float32)


def reference(case, dtype=np.int16):
    """the reference's result for every item of a case, as a list"""
    x = case["x"] if dtype == np.int16 else as_float(case["x"])
    return [measure(x[b, :v], case["fs"], case["target"], case["ceiling"]) for b, v in enumerate(case["lengths"])]


# ---- the inputs of tests/test_audio_boundaries_*.py: items past one turn (LD_THREADS = 256, csrc/efts_loudness.hip:24) of the four strided
# loops of loud_decide_kernel: over the segments' peaks (:122), the sub-blocks (:115) and the 400 ms blocks of both gates (:132, :142)
DECIDE_TURN = 256
BOUNDARY_FS = 8000                                                     # the lowest rate: h = 800, the fewest samples per sub-block
BOUNDARY_NAMES = ("segments_257", "blocks_256", "blocks_257", "blocks_258_late", "short")
BOUNDARY_LENGTHS = (256 * SEGMENT + 1, 259 * 800, 260 * 800, 261 * 800 + 123, 40000)


def boundary_case(ceiling):
    """dict(fs, x int16 [5, n], lengths, target, ceiling) at 8000 Hz, full scale behind every length.
    segments_257: 131 073 samples, the smallest item with a segment at index 256; that segment is its last sample, and the item's peak.
    blocks_256 / blocks_257: 259 and 260 sub-blocks: the gates' loops end with a full first turn, and take one block in a second.
    blocks_258_late: 261 sub-blocks and 123 samples; quiet bursts, then from sub-block 256 on the loudest stretch of the item, with the peak
    in it (segment 400 and above): blocks, sub-blocks and peak of the second turn decide loudness and gain.
    short: 40 000 samples, inside every first turn.
    `ceiling` None: the target of -23 LUFS decides every gain; 0.5 with a target of -14 LUFS: the peak does."""
    rng = np.random.default_rng(8000)
    fs = BOUNDARY_FS
    x = np.full((len(BOUNDARY_LENGTHS), max(BOUNDARY_LENGTHS)), 32767, dtype=np.int16)
    for b, n in enumerate(BOUNDARY_LENGTHS):
        s = _bursts(rng, n, fs, loud=0.1 + 0.02 * b, quiet_db=-50.0)
        if b == 0:
            s[-1] = 0.9
        elif b == 3:
            late = 256 * (fs // 10)
            s[late:] = rng.uniform(-0.4, 0.4, size=n - late)
            s[late + 1234] = 0.95
        else:
            s[n // 3] = 0.8
        x[b, :n] = _quantise(s)
    x.setflags(write=False)
    return dict(fs=fs, x=x, lengths=list(BOUNDARY_LENGTHS), target=-23.0 if ceiling is None else -14.0, ceiling=ceiling)
