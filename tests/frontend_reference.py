"""The definition of the log-mel front-end (nntts/datasets/meldataset.py:49-82, the zero padding of TextMelCollate), restated in numpy float64, the
layouts its kernels hand to each other, an fp32 transcription of every stage (torch on the CPU, torch.stft for the transform: the yardstick
tests/kernel_check.py asks for), and the inputs that tests/test_frontend_reference_cpu.py and tests/test_frontend_kernels_gpu.py share.

Only the window is fp32 (the definition rounds it once, like stft_reference.window); samples, transform, magnitudes, filterbank sums and the log
are float64.  Plain module: it imports neither the package nor oracle/, so the filterbank is written out here a second time.
"""
import functools

import numpy as np
import torch

SR, N_FFT, HOP = 22050, 1024, 256
MAG_EPS, CLAMP, MAX_WAV = 1e-9, 1e-5, 32768.0
EPS = 2.0 ** -23
# the constants of the fused kernel's filterbank table and of the fast radix kernel's (csrc/efts_frontend.hip: FF_CB, FF_WIDE, LM_CB)
FF_CB, FF_WIDE, LM_CB = 2560, 64, 2048
SLANEY = ((80, 8000.0), (64, 11025.0), (40, 4000.0), (72, 7600.0))       # test_fused_fft_launch_on_other_filterbanks_and_frame_counts


# ---- the definition
def window(n_fft):
    """periodic hann, rounded to fp32 once"""
    i = np.arange(n_fft, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / n_fft)).astype(np.float32)


def as_float64(x):
    """int16 PCM times 1 / max_wav_value, fp32 as it is"""
    x = np.asarray(x)
    return x.astype(np.float64) / MAX_WAV if x.dtype == np.int16 else x.astype(np.float64)


def frame_count(L, hop=HOP):
    return L // hop


def frames(x, n_fft=N_FFT, hop=HOP):
    """windowed frames [T, n_fft] of one item: reflect padding by (n_fft - hop) / 2 without edge repeat, T = L // hop"""
    x = as_float64(x)
    pad = (n_fft - hop) // 2
    assert len(x) > pad
    T = frame_count(len(x), hop)
    padded = np.pad(x, pad, mode="reflect")
    idx = hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :]
    return padded[idx] * window(n_fft).astype(np.float64)[None, :]


def spectrum(x, n_fft=N_FFT, hop=HOP):
    """complex [T, n_fft / 2 + 1]"""
    return np.fft.rfft(frames(x, n_fft, hop), axis=1)


def magnitude(spec):
    return np.sqrt(spec.real ** 2 + spec.imag ** 2 + MAG_EPS)


def mel_energy(mag, basis):
    """[T, n_mels] before the clamp and the log"""
    return mag @ np.asarray(basis, dtype=np.float64).T


def log_clamp(v):
    return np.log(np.maximum(v, CLAMP))


def logmel(x, basis, n_fft=N_FFT, hop=HOP):
    return log_clamp(mel_energy(magnitude(spectrum(x, n_fft, hop)), basis))


def pad_rows(rows, T):
    """rows [t, C] of one item -> [T, C], zeros (AFTER the log) at and past the item's frame count; rows past T are dropped"""
    out = np.zeros((T, rows.shape[1]))
    n = min(T, rows.shape[0])
    out[:n] = rows[:n]
    return out


def spectrum_norm(mag):
    """||X_t||_2 over all n_fft bins from the n_fft / 2 + 1 kept magnitudes (the 1e-9 under the root only adds to it)"""
    return np.sqrt(2.0 * (mag ** 2).sum(axis=1) - mag[:, 0] ** 2 - mag[:, -1] ** 2)


def cell_bound(mag, steps):
    """the per-cell bound of log(max(|X[f]|, clamp)) read through a one-hot filter, [T, n_bins]; `steps` = log2 N for the FFT, R for the
    radix recombination.  See the docstring of tests/test_frontend_kernels_gpu.py."""
    tol_mag = EPS * (steps + 4) * spectrum_norm(mag)[:, None] + 4 * EPS * mag
    cl = np.maximum(mag, CLAMP)
    return tol_mag / cl + 4 * EPS * (1.0 + np.abs(np.log(cl)))


def mel_cell_bound(mag, basis, steps):
    """the same for a whole filter, [T, n_mels]: the magnitudes' bounds weighted by the (non-negative) filter, eps (n + 2) of the sum for its n
    products and additions in any order, then the clamp and the log as in cell_bound"""
    b = np.asarray(basis, dtype=np.float64)
    tol_mag = EPS * (steps + 4) * spectrum_norm(mag)[:, None] + 4 * EPS * mag
    mel = mag @ b.T
    n = (b != 0).sum(axis=1)
    cl = np.maximum(mel, CLAMP)
    return (tol_mag @ b.T + EPS * (n + 2)[None, :] * mel) / cl + 4 * EPS * (1.0 + np.abs(np.log(cl)))


# ---- the layouts the kernels exchange
def deinterleave_index(n_fft, R):
    """col[k] = (k mod R) * (n_fft / R) + k // R: the column that holds sample k"""
    k = np.arange(n_fft)
    return (k % R) * (n_fft // R) + k // R


def deinterleave(fr, R):
    out = np.empty_like(fr)
    out[..., deinterleave_index(fr.shape[-1], R)] = fr
    return out


def radix_rows(fr, R):
    """[.., n_fft] frames -> [.., n_fft] radix-R spectrum rows: block p = [re Y_p[0 .. M/2] | im Y_p[1 .. M/2 - 1]], Y_p the real M-point DFT of x[R j + p]"""
    N = fr.shape[-1]
    M = N // R
    out = np.empty(fr.shape, dtype=np.float64)
    for p in range(R):
        Y = np.fft.rfft(fr[..., p::R], axis=-1)
        out[..., p * M:p * M + M // 2 + 1] = Y.real
        out[..., p * M + M // 2 + 1:(p + 1) * M] = Y.imag[..., 1:M // 2]
    return out


def twiddles(R, n_fft):
    """[R, n_bins, 2] = (cos, sin)(2 pi p f / n_fft)"""
    pf = np.arange(R, dtype=np.float64)[:, None] * np.arange(n_fft // 2 + 1, dtype=np.float64)[None, :]
    return np.stack([np.cos(2.0 * np.pi * pf / n_fft), np.sin(2.0 * np.pi * pf / n_fft)], axis=-1)


def recombine(rows, R, tw=None):
    """radix rows [.., n_fft] -> complex spectrum [.., n_bins]: X[f] = sum_p (cos - i sin)(2 pi p f / N) Y_p[f mod M], Y_p[M - g] = conj Y_p[g]"""
    rows = np.asarray(rows, dtype=np.float64)
    N = rows.shape[-1]
    M, nb = N // R, N // 2 + 1
    tw = twiddles(R, N) if tw is None else np.asarray(tw, dtype=np.float64)
    f = np.arange(nb)
    g = f % M
    flip = g > M // 2
    g = np.where(flip, M - g, g)
    X = np.zeros(rows.shape[:-1] + (nb,), dtype=np.complex128)
    for p in range(R):
        blk = rows[..., p * M:(p + 1) * M]
        im = np.zeros(rows.shape[:-1] + (M // 2 + 1,))
        im[..., 1:M // 2] = blk[..., M // 2 + 1:]
        Y = blk[..., g] + 1j * np.where(flip, -1.0, 1.0) * im[..., g]
        X += (tw[p, :, 0] - 1j * tw[p, :, 1]) * Y
    return X


# ---- the fp32 transcription of every stage (torch, CPU)
def frames32(x32, n_fft=N_FFT, hop=HOP):
    pad = (n_fft - hop) // 2
    y = torch.nn.functional.pad(torch.from_numpy(np.array(x32, dtype=np.float32))[None, None], (pad, pad), mode="reflect")[0, 0]
    return y.unfold(0, n_fft, hop)[:len(x32) // hop] * torch.from_numpy(window(n_fft))


def spectrum32(x32, n_fft=N_FFT, hop=HOP):
    """torch.stft, the call the definition itself makes: complex64 [T, n_bins]"""
    pad = (n_fft - hop) // 2
    y = torch.nn.functional.pad(torch.from_numpy(np.array(x32, dtype=np.float32))[None, None], (pad, pad), mode="reflect")[0]
    spec = torch.stft(y, n_fft, hop_length=hop, win_length=n_fft, window=torch.from_numpy(window(n_fft)), center=False, normalized=False,
                      onesided=True, return_complex=True)[0]
    return spec.t()


def logmel_of_spectrum32(re, im, basis):
    """re, im float32 [T, n_bins] -> log-mel float32 [T, n_mels]"""
    mag = torch.sqrt(re * re + im * im + torch.tensor(MAG_EPS, dtype=torch.float32))
    return torch.log(torch.clamp(mag @ torch.from_numpy(np.array(basis, dtype=np.float32)).t(), min=CLAMP))


def logmel32(x32, basis, n_fft=N_FFT, hop=HOP):
    s = spectrum32(x32, n_fft, hop)
    return logmel_of_spectrum32(s.real.contiguous(), s.imag.contiguous(), basis)


def recombine32(rows32, R, tw32):
    """the radix recombination in float32, term after term: (re, im) float32 [.., n_bins]"""
    rows = torch.from_numpy(np.array(rows32, dtype=np.float32))
    tw = torch.from_numpy(np.array(tw32, dtype=np.float32))
    N = rows.shape[-1]
    M, nb = N // R, N // 2 + 1
    f = np.arange(nb)
    g = f % M
    flip = g > M // 2
    g = np.where(flip, M - g, g)
    sgn = torch.from_numpy(np.where(flip, -1.0, 1.0).astype(np.float32))
    xr = torch.zeros(rows.shape[:-1] + (nb,))
    xi = torch.zeros(rows.shape[:-1] + (nb,))
    for p in range(R):
        blk = rows[..., p * M:(p + 1) * M]
        im = torch.zeros(rows.shape[:-1] + (M // 2 + 1,))
        im[..., 1:M // 2] = blk[..., M // 2 + 1:]
        yr, yi = blk[..., g], sgn * im[..., g]
        xr = xr + tw[p, :, 0] * yr + tw[p, :, 1] * yi
        xi = xi + tw[p, :, 0] * yi - tw[p, :, 1] * yr
    return xr, xi


# ---- filterbanks
def slaney(n_mels=80, fmax=8000.0, sr=SR, n_fft=N_FFT, fmin=0.0):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) with htk=False, norm='slaney', from the published definition: float32 [n_mels, n_bins]"""
    def to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-10) / 1000.0) * (27.0 / np.log(6.4)), f * 3.0 / 200.0)

    def to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= 15.0, 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)), m * 200.0 / 3.0)

    bins = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    edges = to_hz(np.linspace(to_mel(fmin), to_mel(fmax), n_mels + 2))
    fb = np.zeros((n_mels, bins.size))
    for m in range(n_mels):
        lo, ce, hi = edges[m], edges[m + 1], edges[m + 2]
        fb[m] = np.clip(np.minimum((bins - lo) / (ce - lo), (hi - bins) / (hi - ce)), 0.0, None) * (2.0 / (hi - lo))
    return fb.astype(np.float32)


def ranges_of(basis):
    """[n_mels, 2] int32: first non-zero bin and one past the last; (0, 0) for an empty filter"""
    rng = np.zeros((basis.shape[0], 2), dtype=np.int32)
    for m in range(basis.shape[0]):
        nz = np.nonzero(basis[m])[0]
        rng[m] = (nz[0], nz[-1] + 1) if nz.size else (0, 0)
    return rng


def fused_table_floats(ranges):
    """what the fused kernel's filterbank table needs for these spans: S0 * min(n_mels, 64) + 4 * SQ * (n_mels - 64) floats, with the kernel's
    w0 / w1 (4-tap steps of the widest one-lane / four-lane filter) and its odd strides S0 = 4 (w0 | 1), SQ = 4 (w1 | 1)"""
    n = ranges[:, 1] - ranges[:, 0]
    w0 = int(((n[:FF_WIDE] + 3) >> 2).max()) if len(n) else 0
    w1 = int(((n[FF_WIDE:] + 15) >> 4).max()) if len(n) > FF_WIDE else 0
    S0, SQ = 4 * (w0 | 1), 4 * (w1 | 1)
    return S0 * min(len(n), FF_WIDE) + 4 * SQ * max(len(n) - FF_WIDE, 0)


@functools.lru_cache(maxsize=None)
def onehot_banks(n_mels=80, n_bins=513):
    """list of (basis [n_mels, n_bins], ranges [n_mels, 2]): a filter is one-hot with ranges (f, f + 1), or empty with ranges (0, 0) once the
    bins of its slot kind are used up.  Across the list every bin appears exactly once in a one-lane slot (m < 64) and exactly once in a
    four-lane slot (m >= 64); bank i holds bins 64 i .. in its one-lane slots and bins 16 i .. (n_mels - 64 per bank) in its four-lane ones,
    so a bin meets two different slots, lanes and neighbours."""
    narrow, wide = min(n_mels, FF_WIDE), max(n_mels - FF_WIDE, 0)
    nb = max(-(-n_bins // narrow), -(-n_bins // wide) if wide else 0)
    banks = []
    for i in range(nb):
        basis = np.zeros((n_mels, n_bins), dtype=np.float32)
        rng = np.zeros((n_mels, 2), dtype=np.int32)
        for m in range(n_mels):
            f = narrow * i + m if m < FF_WIDE else wide * i + (m - FF_WIDE)
            if f < n_bins:
                basis[m, f] = 1.0
                rng[m] = (f, f + 1)
        basis.setflags(write=False)
        rng.setflags(write=False)
        banks.append((basis, rng))
    return tuple(banks)


def _bank_from_spans(spans, n_bins, seed):
    rng = np.random.default_rng(seed)
    basis = np.zeros((len(spans), n_bins), dtype=np.float32)
    for m, (lo, hi) in enumerate(spans):
        if hi > lo:
            w = rng.uniform(0.5, 1.0, hi - lo)
            basis[m, lo:hi] = (0.15 * w / w.sum()).astype(np.float32)       # row sum 0.15: silence (|X| = sqrt(1e-9)) stays below clamp / 2
    ranges = np.array(spans, dtype=np.int32).reshape(-1, 2)
    basis.setflags(write=False)
    ranges.setflags(write=False)
    return basis, ranges


RAGGED_NARROW = ((1, 3, 4, 5, 27), (1, 3, 4))
RAGGED_WIDE = ((1, 15, 16, 17), (1, 15, 16, 17, 63, 64, 65, 144))


@functools.lru_cache(maxsize=None)
def ragged_bank(which=0, n_bins=513):
    """(basis [80, n_bins], ranges [80, 2]): non-negative random weights on spans of ragged lengths, one empty filter (0, 0) of each slot kind, a
    span that starts at bin 0 and one that ends at the last bin in each slot kind.

    The fused kernel's table holds S0 * 64 + 4 * SQ * 16 <= 2560 floats, S0 = 4 (w0 | 1), SQ = 4 (w1 | 1), so (w0 | 1) + (w1 | 1) <= 10: a
    one-lane span of 27 (w0 = 7) and a four-lane span of 144 (w1 = 9) can not share a bank (4096 floats).  Hence two banks, each filling the
    table to its last float: `which` = 0 has one-lane spans 1, 3, 4, 5, 27 and four-lane spans 1, 15, 16, 17 (28 * 64 + 48 * 16 = 2560);
    `which` = 1 has one-lane spans 1, 3, 4 and four-lane spans 1, 15, 16, 17, 63, 64, 65, 144 (4 * 64 + 144 * 16 = 2560)."""
    rng = np.random.default_rng(1000 + which)
    nl, wl = RAGGED_NARROW[which], RAGGED_WIDE[which]
    lens = [nl[m % len(nl)] for m in range(FF_WIDE)] + [wl[m % len(wl)] for m in range(16)]
    spans = []
    for m, n in enumerate(lens):
        n = min(n, n_bins)
        lo = int(rng.integers(0, n_bins - n + 1))
        spans.append((lo, lo + n))
    for base, count in ((0, FF_WIDE), (FF_WIDE, 16)):
        first, last, empty = base, base + count - 1, base + 5
        spans[first] = (0, spans[first][1] - spans[first][0])                                   # starts at bin 0
        spans[last] = (n_bins - (spans[last][1] - spans[last][0]), n_bins)                      # ends at the last bin
        spans[empty] = (0, 0)
    # the widest span of each kind must survive the three replacements above
    return _bank_from_spans(spans, n_bins, 2000 + which)


@functools.lru_cache(maxsize=None)
def fat_bank(n_bins=513):
    """128 filters of 20 bins each, spread over all bins: 2560 weights > LM_CB = 2048, the fast radix kernel reads them from memory"""
    spans = [(int(round(m * (n_bins - 20) / 127.0)), int(round(m * (n_bins - 20) / 127.0)) + 20) for m in range(128)]
    return _bank_from_spans(spans, n_bins, 3000)


@functools.lru_cache(maxsize=None)
def slaney_bank(n_mels=80, fmax=8000.0, n_fft=N_FFT):
    basis = slaney(n_mels, fmax, n_fft=n_fft)
    ranges = ranges_of(basis)
    basis.setflags(write=False)
    ranges.setflags(write=False)
    return basis, ranges


# ---- inputs
def signal(L, seed):
    """(pcm int16, the same values as fp32): two sines (220 Hz, 3100 Hz) plus 0.02-sigma noise, rounded to the int16 grid"""
    rng = np.random.default_rng(seed)
    n = np.arange(L, dtype=np.float64)
    y = 0.3 * np.sin(2 * np.pi * 220.0 / SR * n) + 0.2 * np.sin(2 * np.pi * 3100.0 / SR * n + 0.7) + 0.02 * rng.standard_normal(L)
    pcm = np.round(y * MAX_WAV).clip(-32768, 32767).astype(np.int16)
    return pcm, (pcm.astype(np.float32) / np.float32(MAX_WAV)).astype(np.float32)


def silence(L):
    pcm = np.zeros(L, dtype=np.int16)
    return pcm, pcm.astype(np.float32)


def square(L, period=97):
    """full-scale int16 square wave: +32767 over the first 48 samples of a period, -32768 over the other 49"""
    pcm = np.where(np.arange(L) % period < period // 2, 32767, -32768).astype(np.int16)
    return pcm, (pcm.astype(np.float32) / np.float32(MAX_WAV)).astype(np.float32)


def stage_frames(n_fft):
    """the input of the single-stage tests, float64 windowed frames [5, n_fft]: four frames of a signal and one all-zero row"""
    pcm, _ = signal(4 * n_fft + 3, 3)
    return np.concatenate([frames(pcm, n_fft, n_fft // 4)[3:7], np.zeros((1, n_fft))])


# the items of the fused kernel's tests: one frame with an empty partner; at t0 = 2 the pair of the 1408-sample item takes the constant-offset
# loads (128 + 20 * 64 = 1408 <= L) and that of the 1407-sample item the reflecting ones; an odd length over several pairs; silence; full scale
SIGNAL_LENGTHS = (385, 1408, 1407, 4099)
ITEM_NAMES = ("385", "1408", "1407", "4099", "silence", "square")
SILENT, SQUARE = 4, 5


@functools.lru_cache(maxsize=None)
def items():
    """tuple of (name, pcm int16, fp32) -- read-only"""
    out = [(str(L),) + signal(L, 100 + i) for i, L in enumerate(SIGNAL_LENGTHS)]
    out.append(("silence",) + silence(1300))
    out.append(("square",) + square(2051))
    for _, p, f in out:
        p.setflags(write=False)
        f.setflags(write=False)
    return tuple(out)


def batch(item_list, fill_f32=np.nan, fill_i16=32767):
    """(pcm int16 [B, Lmax], fp32 [B, Lmax], lengths): 32767 / NaN behind every item's length"""
    lengths = [len(p) for _, p, _ in item_list]
    pcm = np.full((len(item_list), max(lengths)), fill_i16, dtype=np.int16)
    f32 = np.full((len(item_list), max(lengths)), fill_f32, dtype=np.float32)
    for b, (_, p, f) in enumerate(item_list):
        pcm[b, :len(p)] = p
        f32[b, :len(f)] = f
    return pcm, f32, lengths


# (item, bank) pairs of the fused kernel's whole-bank test whose fp32 transcription is itself too far from float64 for kernel_check's bound
# (a one-bin filter between two harmonics of the full-scale square wave: |X[f]| = 3e-4 under a spectrum of norm 1.6e4); they are held to
# mel_cell_bound alone, like every other cell is in addition.  Pinned by tests/test_frontend_reference_cpu.py.
BANK_NAMES = ("slaney80_8000", "slaney64_11025", "slaney40_4000", "slaney72_7600", "ragged0", "ragged1")
ILL_CONDITIONED = (("square", "ragged1"),)


def whole_banks():
    return tuple(zip(BANK_NAMES, [slaney_bank(n, f) for n, f in SLANEY] + [ragged_bank(0), ragged_bank(1)]))


PERSISTENT_T, PERSISTENT_MAX_B = 900, 16


@functools.lru_cache(maxsize=None)
def persistent_items(B):
    """B rotations of one signal of PERSISTENT_T frames, lengths shortened by 0 .. 4 hops and a few samples"""
    base, _ = signal(PERSISTENT_T * HOP, 7)
    out = []
    for b in range(B):
        pcm = np.roll(base, 4099 * b)[:PERSISTENT_T * HOP - (b % 5) * HOP - 3 * (b % 2)].copy()
        f = (pcm.astype(np.float32) / np.float32(MAX_WAV)).astype(np.float32)
        pcm.setflags(write=False)
        f.setflags(write=False)
        out.append((f"rot{b}", pcm, f))
    return tuple(out)


def persistent_batch_size(cus):
    """the smallest B with B * ceil(T / 2) > 12 * CUs: beyond the launch's 3 * CUs blocks of 4 waves, every wave works through several pairs"""
    return 12 * cus // ((PERSISTENT_T + 1) // 2) + 1
