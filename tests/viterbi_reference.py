"""numpy restatement, in 64-bit integers and without renormalisation, of the pitch smoother's definition in include/efts_abi.h ("Smoothing the
pitch across frames").  Written from the header; it never imports the product.  Inputs are the d' rows as float32, the four costs as floats,
tau_min and tau_max.  Also holds the "octave-up glitch" signal of the tests."""
import numpy as np

Q = 65536
DEFAULT_COSTS = dict(unvoiced_cost=0.15, octave_cost=0.02, jump_cost=0.35, vuv_cost=0.14)


def log2_table(tau_max):
    """int32 [tau_max + 1]: lg[k] = rint(log2(k) Q) for k >= 1, float64; entry 0 is unused"""
    lg = np.zeros(tau_max + 1, dtype=np.int64)
    lg[1:] = np.rint(np.log2(np.arange(1, tau_max + 1, dtype=np.float64)) * Q).astype(np.int64)
    return lg


def cost_q(value):
    return int(np.rint(np.float64(value) * Q))


def quantise(x):
    """q(x) on float32 input, float32 arithmetic: x < 4 ? rint(x * 65536) : 4 Q; NaN and +inf land on 4 Q, anything at or below -4 on -4 Q"""
    x = np.asarray(x, dtype=np.float32)
    inside = (x < np.float32(4.0)) & (x > np.float32(-4.0))
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = np.rint(np.where(inside, x, np.float32(0.0)) * np.float32(65536.0))
    out = np.where(inside, scaled, np.where(x <= np.float32(-4.0), -4.0 * Q, 4.0 * Q))
    return out.astype(np.int64)


def viterbi_reference(cmnd, tau_min, tau_max, unvoiced_cost=0.15, octave_cost=0.02, jump_cost=0.35, vuv_cost=0.14):
    """cmnd: float32 [n, tau_max + 1], the n frames of ONE item.  Returns (lag int64 [n] with 0 for unvoiced, states int64 [n])."""
    cmnd = np.asarray(cmnd, dtype=np.float32)
    n = cmnd.shape[0]
    assert cmnd.ndim == 2 and cmnd.shape[1] == tau_max + 1 and 2 <= tau_min < tau_max - 1 <= 1023
    S = tau_max - tau_min
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    uq, oq, jq, vq = (cost_q(c) for c in (unvoiced_cost, octave_cost, jump_cost, vuv_cost))
    assert all(0 <= c <= 16 * Q for c in (uq, oq, jq, vq))
    lg = log2_table(tau_max)
    lgs = lg[tau_min:tau_max]                                                     # lg of state s
    octave = (oq * (lgs - lg[tau_min])) >> 16
    trans = np.empty((S + 1, S + 1), dtype=np.int64)                              # trans[p, s]
    trans[:S, :S] = (jq * np.abs(lgs[None, :] - lgs[:, None])) >> 16
    trans[S, :S] = vq
    trans[:S, S] = vq
    trans[S, S] = 0

    def obs(t):
        return np.concatenate([quantise(cmnd[t, tau_min:tau_max]) + octave, np.array([uq], dtype=np.int64)])

    C = obs(0)
    back = np.zeros((n, S + 1), dtype=np.int64)
    for t in range(1, n):
        total = C[:, None] + trans                                                # [p, s]
        back[t] = total.argmin(axis=0)                                            # the first, i.e. lowest, index among equal minima
        C = obs(t) + total.min(axis=0)
    states = np.zeros(n, dtype=np.int64)
    states[n - 1] = int(C.argmin())
    for t in range(n - 1, 0, -1):
        states[t - 1] = back[t, states[t]]
    return np.where(states < S, states + tau_min, 0), states


def outputs_reference(cmnd, lag, sr, tau_min, tau_max):
    """(f0, aperiodicity, den) in float64 from the float32 d' rows and the path's lags: the parabola at the lag itself, the row minimum
    (NaN passed over) for an unvoiced frame.  den is the parabola's denominator (NaN for an unvoiced frame)."""
    cmnd = np.asarray(cmnd, dtype=np.float32)
    n = cmnd.shape[0]
    f0, ap, dens = np.zeros(n), np.zeros(n), np.full(n, np.nan)
    for t in range(n):
        k = int(lag[t])
        if k == 0:
            ap[t] = np.fmin.reduce(cmnd[t, tau_min:tau_max].astype(np.float64))
            continue
        s0, s1, s2 = (np.float64(cmnd[t, k + o]) for o in (-1, 0, 1))
        with np.errstate(invalid="ignore", divide="ignore"):
            den = (s0 - s1) + (s2 - s1)
            shift = 0.0 if den == 0.0 else 0.5 * (s0 - s2) / den
        shift = -1.0 if np.isnan(shift) else min(1.0, max(-1.0, shift))
        f0[t], ap[t], dens[t] = sr / (k + shift), s1, den
    return f0, ap, dens


GLITCH_SAMPLES, GLITCH_SR = 8000, 22050


def glitch_signal():
    """150 Hz with a second harmonic that takes over on samples 3000 .. 4199: plain YIN flips an octave up for a few frames there"""
    n, sr = GLITCH_SAMPLES, GLITCH_SR
    t = np.arange(n) / sr
    w = np.zeros(n)
    w[3000:4200] = 1.0
    x = (1.0 - 0.93 * w) * np.sin(2.0 * np.pi * 150.0 * t) + (0.3 + 0.7 * w) * np.sin(2.0 * np.pi * 300.0 * t + 0.4)
    return 0.9 * x / np.abs(x).max()
