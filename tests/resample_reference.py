"""float64 numpy restatement of the sample-rate converter (efficient_tts_amd/resample.py, csrc/efts_resample.hip): h(tau) is evaluated
directly for every output sample and every tap -- no table, no polyphase indexing, nothing imported from the package.

    g = gcd(src, dst), L = dst / g, M = src / g;  fc = rolloff * min(1, dst / src);  W = ceil(Z / fc)
    h(tau) = fc sinc(fc tau) I0(beta sqrt(1 - (fc tau / Z)^2)) / I0(beta) for |fc tau| < Z, 0 otherwise
    y[n] = sum over k = -W .. W of x[i0 + k] h(p / L - k),  i0 = floor(n M / L), p = (n M) mod L,  x = 0 outside [0, len)
"""
import math

import numpy as np

QUALITIES = {"best": (64, 14.77, 0.9476), "fast": (16, 8.555, 0.85)}


def geometry(src, dst, quality):
    Z, beta, rolloff = QUALITIES[quality]
    g = math.gcd(src, dst)
    L, M = dst // g, src // g
    fc = rolloff * min(1.0, dst / src)
    W = int(math.ceil(Z / fc))
    return L, M, W, fc, Z, beta


def kernel(tau, fc, Z, beta):
    """h(tau), tau in source samples (any shape), float64"""
    u = fc * np.asarray(tau, dtype=np.float64)
    win = np.i0(beta * np.sqrt(np.clip(1.0 - (u / Z) ** 2, 0.0, None))) / np.i0(beta)
    return np.where(np.abs(u) < Z, fc * np.sinc(u) * win, 0.0)


def length(n, src, dst):
    g = math.gcd(src, dst)
    L, M = dst // g, src // g
    return (n * L + M - 1) // M


def table(src, dst, quality):
    """h(p / L - k) as [L, 2 W + 1], float64: the formula the product's fp32 table is compared with"""
    L, M, W, fc, Z, beta = geometry(src, dst, quality)
    tau = np.arange(L, dtype=np.float64)[:, None] / L - np.arange(-W, W + 1, dtype=np.float64)[None, :]
    return kernel(tau, fc, Z, beta)


def resample(x, src, dst, quality, outputs=None, fp32_taps=False, chunk=4096):
    """y[n] for n in `outputs` (default: all of them), float64 sums.  fp32_taps: the taps rounded to fp32 first (what the device holds)."""
    x = np.asarray(x, dtype=np.float64)
    L, M, W, fc, Z, beta = geometry(src, dst, quality)
    n_all = np.arange(length(x.shape[0], src, dst), dtype=np.int64) if outputs is None else np.asarray(outputs, dtype=np.int64)
    y = np.zeros(n_all.shape[0], dtype=np.float64)
    k = np.arange(-W, W + 1, dtype=np.int64)
    for lo in range(0, n_all.shape[0], chunk):
        n = n_all[lo:lo + chunk]
        pos = n * M
        i0, p = pos // L, pos % L
        taps = kernel(p[:, None].astype(np.float64) / L - k[None, :], fc, Z, beta)
        if fp32_taps:
            taps = taps.astype(np.float32).astype(np.float64)
        idx = i0[:, None] + k[None, :]
        ok = (idx >= 0) & (idx < x.shape[0])
        y[lo:lo + chunk] = (np.where(ok, x[np.clip(idx, 0, max(x.shape[0] - 1, 0))] if x.shape[0] else 0.0, 0.0) * taps).sum(axis=1)
    return y


def bound(src, dst, quality, peak=1.0):
    """K * 2^-23 * max over p of sum_k |h[p][k]| * max |x|: the fp32 chain of K fused multiply-adds against exact sums"""
    t = np.abs(table(src, dst, quality))
    return t.shape[1] * 2.0 ** -23 * t.sum(axis=1).max() * peak
