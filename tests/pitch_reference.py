"""Float64 numpy restatement of the pitch tracker (efficient_tts_amd/pitch.py, csrc/efts_pitch.hip), of the warping path of `score.dtw_path`
and of `score.F0Error`, written from the definitions in include/efts_abi.h and never importing the product.

YIN per frame x[0 .. N - 1], W = N / 2, tau_min = floor(sr / fmax), tau_max = min(W, floor(sr / fmin)) (the library refuses an fmin whose
period exceeds W, so the minimum never bites there):
    d(tau)  = sum_{j < W} (x[j] - x[j + tau])^2,  tau = 1 .. tau_max
    d'(tau) = d(tau) tau / (d(1) + .. + d(tau)), 1 where that sum is 0; d'(0) = 1
    tau     = the smallest lag in [tau_min, tau_max - 1] with d'(tau) < threshold; advanced while tau + 1 <= tau_max - 1 and d'(tau + 1) < d'(tau);
              s0, s1, s2 = d'(tau - 1), d'(tau), d'(tau + 1), den = (s0 - s1) + (s2 - s1), shift = clamp(0.5 (s0 - s2) / den, -1, 1), 0 for den == 0
    f0      = sr / (tau + shift), aperiodicity = s1;  no such lag: f0 = 0, aperiodicity = min d' over [tau_min, tau_max - 1]
Framing: frames = length // hop, pad = (N - hop) / 2, sample s of frame t = audio index t hop - pad + s, reflected: i < 0 -> -i,
i >= length -> 2 (length - 1) - i.
"""
import math

import numpy as np

MARGIN = 1e-3


def lag_range(sr, n_fft, fmin, fmax):
    return int(math.floor(sr / fmax)), int(min(n_fft // 2, math.floor(sr / fmin)))


def frame_indices(length, n_fft, hop):
    """int64 [frames, n_fft]: the audio index behind every sample of every frame"""
    frames, pad = length // hop, (n_fft - hop) // 2
    idx = np.arange(frames, dtype=np.int64)[:, None] * hop - pad + np.arange(n_fft, dtype=np.int64)[None, :]
    idx = np.where(idx < 0, -idx, idx)
    return np.where(idx >= length, 2 * (length - 1) - idx, idx)


def difference(x, tau_max):
    """d [tau_max + 1] of one frame (d[0] = 0)"""
    x = np.asarray(x, dtype=np.float64)
    W = x.shape[0] // 2
    d = np.zeros(tau_max + 1)
    for tau in range(1, tau_max + 1):
        d[tau] = np.sum((x[:W] - x[tau:tau + W]) ** 2)
    return d


def normalise(d):
    """d' [tau_max + 1]: d'(0) = 1"""
    out = np.ones_like(d)
    run = 0.0
    for tau in range(1, d.shape[0]):
        run += d[tau]
        out[tau] = d[tau] * tau / run if run != 0.0 else 1.0
    return out


def decide(dp, sr, tau_min, tau_max, threshold):
    """(tau or 0, f0, aperiodicity, margin) from one frame's d' [tau_max + 1] alone.  margin: the smallest distance in d' of any comparison
    that determined the decision -- d'(tau) < threshold for every lag up to the chosen one (every lag of the range for an unvoiced frame),
    and the comparisons of the walk forward, the one that ended it included."""
    dp = np.asarray(dp, dtype=np.float64)
    margin = np.inf
    tau = 0
    for k in range(tau_min, tau_max):
        margin = min(margin, abs(dp[k] - threshold))
        if dp[k] < threshold:
            tau = k
            break
    if tau == 0:
        return 0, 0.0, float(dp[tau_min:tau_max].min()), margin
    while tau + 1 <= tau_max - 1:
        margin = min(margin, abs(dp[tau + 1] - dp[tau]))
        if not dp[tau + 1] < dp[tau]:
            break
        tau += 1
    s0, s1, s2 = dp[tau - 1], dp[tau], dp[tau + 1]
    den = (s0 - s1) + (s2 - s1)
    shift = 0.0 if den == 0.0 else min(1.0, max(-1.0, 0.5 * (s0 - s2) / den))
    return tau, sr / (tau + shift), float(s1), margin


def yin_reference(audio, length, sr, n_fft, hop, fmin, fmax, threshold):
    """dict of per-frame arrays: d, dp [frames, tau_max + 1], tau, f0, aperiodicity, margin [frames]; audio as the kernel sees it (int16 PCM
    already scaled), cast to float64"""
    audio = np.asarray(audio, dtype=np.float64)
    tau_min, tau_max = lag_range(sr, n_fft, fmin, fmax)
    assert 2 <= tau_min < tau_max - 1
    idx = frame_indices(int(length), n_fft, hop)
    T = idx.shape[0]
    out = dict(d=np.zeros((T, tau_max + 1)), dp=np.zeros((T, tau_max + 1)), tau=np.zeros(T, dtype=np.int64), f0=np.zeros(T), aperiodicity=np.zeros(T),
               margin=np.zeros(T))
    for t in range(T):
        d = difference(audio[idx[t]], tau_max)
        dp = normalise(d)
        out["d"][t], out["dp"][t] = d, dp
        out["tau"][t], out["f0"][t], out["aperiodicity"][t], out["margin"][t] = decide(dp, sr, tau_min, tau_max, threshold)
    return out


def dtw_path_reference(x, y):
    """(cost, path_len, path [path_len, 2] in forward order) of x [Tx, D] against y [Ty, D]: the full matrix, the tie rule of score.py's
    docstring (diagonal, then (i-1, j), then (i, j-1); a later one wins only when strictly smaller), and the back-trace"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    tx, ty = x.shape[0], y.shape[0]
    d2 = np.zeros((tx, ty))
    for k in range(x.shape[1]):
        d2 += (x[:, k, None] - y[None, :, k]) ** 2
    d = np.sqrt(d2)
    A = np.full((tx + 1, ty + 1), np.inf)                  # cell (i, j) lives at [i + 1, j + 1]; the cell in front of (0, 0) is 0
    A[0, 0] = 0.0
    choice = np.zeros((tx, ty), dtype=np.int8)
    for s in range(tx + ty - 1):
        i = np.arange(max(0, s - ty + 1), min(s, tx - 1) + 1)
        j = s - i
        best, c = A[i, j].copy(), np.zeros(i.shape[0], dtype=np.int8)
        for code, a in ((1, A[i, j + 1]), (2, A[i + 1, j])):
            m = a < best
            best[m], c[m] = a[m], code
        A[i + 1, j + 1], choice[i, j] = d[i, j] + best, c
    cells = [(tx - 1, ty - 1)]
    while cells[-1] != (0, 0):
        i, j = cells[-1]
        cells.append(((i - 1, j - 1), (i - 1, j), (i, j - 1))[choice[i, j]])
    path = np.array(cells[::-1], dtype=np.int64)
    return float(A[tx, ty]), path.shape[0], path


def path_is_valid(path, tx, ty):
    path = np.asarray(path, dtype=np.int64)
    if path.ndim != 2 or path.shape[0] < 1 or tuple(path[0]) != (0, 0) or tuple(path[-1]) != (tx - 1, ty - 1):
        return False
    steps = {tuple(s) for s in np.diff(path, axis=0)}
    return steps <= {(1, 1), (1, 0), (0, 1)}


def f0_error_reference(f0_a, f0_b, path):
    """(f0_rmse_cents, vuv_error, voiced_pairs) along path [n, 2]"""
    f0_a, f0_b, path = np.asarray(f0_a, dtype=np.float64), np.asarray(f0_b, dtype=np.float64), np.asarray(path, dtype=np.int64).reshape(-1, 2)
    if path.shape[0] == 0:
        return math.nan, math.nan, 0
    a, b = f0_a[path[:, 0]], f0_b[path[:, 1]]
    both = (a > 0) & (b > 0)
    n = int(both.sum())
    rmse = math.sqrt(float(np.mean((1200.0 * np.log2(a[both] / b[both])) ** 2))) if n else math.nan
    return rmse, float(((a > 0) != (b > 0)).mean()), n


# ---- the inputs shared by tests/test_pitch_cpu.py and tests/test_pitch_gpu.py ----

SR = 22050
TONES = [("fixed 110.25 Hz (200 samples)", 110.25, 110.25), ("fixed 147 Hz (150 samples)", 147.0, 147.0), ("fixed 233.3 Hz", 233.3, 233.3),
         ("fixed 391.7 Hz", 391.7, 391.7), ("glide 120 -> 135 Hz", 120.0, 135.0), ("glide 300 -> 280 Hz", 300.0, 280.0)]
PARTIALS = (1.0, 0.5, 0.25, 0.125)


def tone(f_start, f_end, n, sr=SR):
    """(samples float64 [n] with peak 0.9, instantaneous fundamental [n]): four partials of decaying amplitude on a linear glide"""
    f = np.linspace(f_start, f_end, n)
    phase = 2.0 * np.pi * np.cumsum(f) / sr
    x = sum(a * np.sin((h + 1) * phase + 0.3 * h) for h, a in enumerate(PARTIALS))
    return 0.9 * x / np.abs(x).max(), f


TONE_SAMPLES = 6000
# the largest relative f0 error of yin_reference itself over TONES (n_fft 1024, hop 256, 60 .. 600 Hz, threshold 0.15), on the frames that need
# no reflection, against true_f0: measured by tests/test_pitch_cpu.py, which holds this figure to the measurement (the glide 120 -> 135 Hz sets it)
REFERENCE_TONE_ERROR = 1.08e-3


def inside_frames(n, n_fft, hop):
    """the frames of an n-sample item that need no reflection: every sample of theirs lies inside the item"""
    pad = (n_fft - hop) // 2
    return [t for t in range(n // hop) if t * hop - pad >= 0 and t * hop - pad + n_fft - 1 < n]


def true_f0(f_inst, t, n_fft, hop):
    """the fundamental a frame is held against: the instantaneous one at the middle of the span x[0 .. W + tau) that d(tau) reads at the
    true period tau"""
    start = t * hop - (n_fft - hop) // 2
    mid = start + n_fft // 4
    mid = start + int(round((n_fft // 2 + SR / f_inst[mid]) / 2.0))
    return f_inst[mid]


def stage_batch(n_fft, hop, seed):
    """the ragged batch of the d' and decision tests: (list of float64 arrays, kinds).  No length is a multiple of hop; the last item (all zeros) is one
    sample longer than the shortest the framing admits (pad + 1) and has a single frame; the third repeats one 50-sample period exactly, so its
    d'(50) is 0 in any precision.  The glide stays between 391.7 and 396.5 Hz, periods of
    56.29 .. 55.61 samples: a clean tone's d' valley is shallow in absolute terms, and where the period sits half-way between two lags the
    walk forward compares two nearly equal values -- such frames have no margin (MARGIN) and this glide avoids them"""
    rng = np.random.default_rng(seed)
    pad = (n_fft - hop) // 2
    lengths = [5999, 1901, 2613, pad + 2]
    assert all(n % hop and n > pad for n in lengths) and lengths[3] // hop == 1
    period = tone(SR / 50.0, SR / 50.0, 50)[0]                                     # 441 Hz: one period of 50 samples, repeated exactly
    items = [tone(391.7, 396.5, lengths[0])[0], 0.3 * rng.standard_normal(lengths[1]), np.tile(period, lengths[2] // 50 + 1)[:lengths[2]], np.zeros(lengths[3])]
    return items, ["glide", "noise", "integer-period tone", "zero"]


def as_pcm16(x):
    return np.round(np.asarray(x) * 32767.0).astype(np.int16)
