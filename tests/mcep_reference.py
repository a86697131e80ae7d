"""The definition of the waveform mel-cepstra and of the mel-cepstral distortion (include/efts_abi.h, efficient_tts_amd/mcep.py), restated
in numpy float64 WITHOUT the table: log periodogram -> cepstrum by an inverse real FFT -> Oppenheim's recursion per frame -> c~[1 .. M].  Also
the fp32 yardstick (the same definition through torch.stft, fp32 log and an fp32 matmul on the CPU) and the inputs that tests/test_mcep_cpu.py
and tests/test_mcep_gpu.py share.  Only the window and the table under test are fp32; everything else here is float64."""
import functools

import numpy as np

import stft_reference as ST

N, K, ORDER, ALPHA = 1024, 512, 24, 0.455
CLAMP = 1e-7
MCD_DB = 10.0 * np.sqrt(2.0) / np.log(10.0)
LENGTHS = (0, 512, 513, 1024, 2049, 12345)
CONFIGS = (("fp32", False, 256, 1024), ("int16", True, 256, 1024), ("fp32_hop120_win600", False, 120, 600))      # name, int16, hop, window


def freqt(c, order=ORDER, alpha=ALPHA):
    """c [..., n] -> [..., order + 1]: the all-pass frequency transform (SPTK's freqt), every leading index on its own"""
    c = np.asarray(c, dtype=np.float64)
    g = np.zeros(c.shape[:-1] + (order + 1,))
    beta = 1.0 - alpha * alpha
    for i in range(c.shape[-1] - 1, -1, -1):
        d = g.copy()
        g[..., 0] = c[..., i] + alpha * d[..., 0]
        if order >= 1:
            g[..., 1] = beta * d[..., 0] + alpha * d[..., 1]
        for j in range(2, order + 1):
            g[..., j] = d[..., j - 1] + alpha * (d[..., j] - g[..., j - 1])
    return g


def one_sided_cepstrum(log_mag):
    """c^ [..., K + 1] with ln|X(w_f)| = sum_n c^[n] cos(n w_f), from ln|X| at f = 0 .. K"""
    c = np.fft.irfft(np.asarray(log_mag, dtype=np.float64), n=2 * (log_mag.shape[-1] - 1), axis=-1)[..., :log_mag.shape[-1]]
    c[..., 1:-1] *= 2.0
    return c


def mel_cepstrum_of_log_power(L, order=ORDER, alpha=ALPHA):
    """ln P [..., K + 1] -> c~[1 .. order]"""
    return freqt(one_sided_cepstrum(0.5 * np.asarray(L, dtype=np.float64)), order, alpha)[..., 1:]


def warped_log_magnitude(c_tilde, alpha=ALPHA, bins=K):
    """ln|X| at w_f = pi f / bins, f = 0 .. bins, of the spectrum whose mel-cepstrum is c_tilde[0 ..]"""
    w = np.pi * np.arange(bins + 1) / bins
    wt = w + 2.0 * np.arctan2(alpha * np.sin(w), 1.0 - alpha * np.cos(w))
    return np.cos(np.arange(len(c_tilde))[None, :] * wt[:, None]) @ np.asarray(c_tilde, dtype=np.float64)


def power(x, H, W):
    """P [T, K + 1] of one item, clamped; T = 0 for an item of at most N / 2 samples"""
    return ST.magnitudes(x, N, H, W) ** 2 if ST.frame_count(len(x), N, H) else np.zeros((0, K + 1))


def mel_cepstrum(x, H=256, W=1024, order=ORDER, alpha=ALPHA):
    P = power(x, H, W)
    return mel_cepstrum_of_log_power(np.log(P), order, alpha) if len(P) else np.zeros((0, order))


def frame_distances(a, b):
    """d(t, t), t = 0 .. min(Ta, Tb) - 1"""
    n = min(len(a), len(b))
    return np.sqrt(((a[:n] - b[:n]) ** 2).sum(axis=1))


def aligned_cost(a, b):
    """(cost, count): the sum in frame order, NaN without a frame"""
    d = frame_distances(a, b)
    cost = 0.0
    for v in d:
        cost += float(v)
    return (cost if len(d) else float("nan")), len(d)


# ---- the inputs: a buzz of flat harmonics under every bin plus white noise 40 dB below it.  Almost no cell of such a signal comes near the
# clamp, with one exception that no level cures: the first frame is centred on sample 0, so reflect padding makes it even, its spectrum is
# real up to a linear phase, and a real spectrum crosses zero between bins.  The seeds below were searched (tests/test_mcep_cpu.py checks the
# outcome) so that every cell of every frame, at both resolutions of CONFIGS, holds at least 1e-5 = 100 x the clamp.
SEEDS = {0: (0, 0, 1, 3, 4, 2), 1: (0, 0, 1, 9, 3, 3)}             # variant -> one seed per item of LENGTHS


def signal(L, item, seed, noise_db=-40.0):
    rng = np.random.default_rng(seed)
    n = np.arange(L, dtype=np.float64)
    f0 = 17.0 + 0.45 * item                                            # below the bin spacing of 21.5 Hz: every bin lies in a main lobe
    ks = np.arange(1, int(11025.0 / f0))
    phases = rng.uniform(0.0, 2.0 * np.pi, len(ks))
    x = np.sin(2.0 * np.pi * f0 / 22050.0 * np.outer(n, ks) + phases[None, :]).sum(axis=1) if L else np.zeros(0)
    x *= np.sqrt(0.03 / (0.5 * len(ks)))                               # power 0.03: peaks stay inside the int16 range
    return x + np.sqrt(0.03 * 10.0 ** (noise_db / 10.0)) * rng.standard_normal(L)


def pcm(L, item, seed):
    return np.round(signal(L, item, seed) * ST.MAX_WAV).clip(-32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def batch(pcm16=False, variant=0):
    """(x [B, max] fp32 or int16, lengths): item b holds its signal on the int16 grid (the fp32 batch is the int16 one times 2^-15, exactly),
    zeros behind it.  variant 1: other signals of the same lengths, the partner in the distortion tests"""
    x = np.zeros((len(LENGTHS), max(LENGTHS)), dtype=np.int16)
    for b, L in enumerate(LENGTHS):
        x[b, :L] = pcm(L, b + 6 * variant, SEEDS[variant][b])
    return (x if pcm16 else (x.astype(np.float32) / np.float32(ST.MAX_WAV))), np.asarray(LENGTHS, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def reference_batch(pcm16=False, H=256, W=1024, variant=0):
    """per item: (mc [T, ORDER] float64, the smallest power cell or inf)"""
    x, lengths = batch(pcm16, variant)
    out = []
    for b, L in enumerate(lengths):
        P = power(x[b, :L], H, W)
        out.append((mel_cepstrum_of_log_power(np.log(P)) if len(P) else np.zeros((0, ORDER)), float(P.min()) if P.size else float("inf")))
    return out


def yardstick_item(x, H, W, table32):
    """the same definition in fp32 on the CPU: torch.stft, fp32 log, fp32 matmul with the fp32 table -> [T, order] float32"""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(x))
    x = x.to(torch.float32) * (1.0 / ST.MAX_WAV) if x.dtype == torch.int16 else x
    if ST.frame_count(len(x), N, H) == 0:
        return np.zeros((0, table32.shape[0]), dtype=np.float32)
    spec = torch.stft(x, N, hop_length=H, win_length=W, window=torch.from_numpy(ST.window(W)), center=True, pad_mode="reflect", return_complex=True)
    P = torch.clamp(spec.real ** 2 + spec.imag ** 2, min=CLAMP)
    return (torch.log(P).T.contiguous() @ torch.from_numpy(table32).T.contiguous()).numpy()


@functools.lru_cache(maxsize=None)
def yardstick(pcm16=False, H=256, W=1024):
    """max |fp32 yardstick - float64 reference| over the batch and the all-zero item of 2049 samples"""
    from efficient_tts_amd.mcep import mcep_table
    table32 = mcep_table(N, ORDER, ALPHA).astype(np.float32)
    x, lengths = batch(pcm16)
    ref = reference_batch(pcm16, H, W)
    worst = 0.0
    for b, L in enumerate(lengths):
        if len(ref[b][0]):
            worst = max(worst, float(np.abs(yardstick_item(x[b, :L], H, W, table32).astype(np.float64) - ref[b][0]).max()))
    zero = np.zeros(2049, dtype=x.dtype)
    return max(worst, float(np.abs(yardstick_item(zero, H, W, table32).astype(np.float64) - mel_cepstrum(zero, H, W)).max()))


# ---- the inputs of tests/test_audio_boundaries_*.py: items whose frames end on either side of what one workgroup of logspec_project_kernel
# takes (LP_UPB = 64 pairs, 128 frames: csrc/efts_mcep.hip:28), and frame sequences on either side of one step of frame_dist_kernel
# (FD_CHUNK = 1024 frames: csrc/efts_mcep.hip:117)
FRAMES_PER_WORKGROUP, DIST_CHUNK = 128, 1024
BOUNDARY_FRAMES = (127, 128, 129, 130)
BOUNDARY_CONFIGS = (("fp32", False, 256, 1024), ("int16", True, 256, 1024), ("fp32_hop120_win600", False, 120, 600), ("int16_hop120_win600", True, 120, 600))
BOUNDARY_REST = {256: (17, 0, 255, 100), 120: (7, 0, 119, 60)}        # len = H (T - 1) + r, 0 <= r < H
BOUNDARY_SEEDS = (2, 5, 0, 0)                                         # searched like SEEDS: every power cell at least 1e-5 at both hops


def boundary_lengths(H):
    return tuple(H * (T - 1) + r for T, r in zip(BOUNDARY_FRAMES, BOUNDARY_REST[H]))


@functools.lru_cache(maxsize=None)
def _boundary_pcm(item):
    return pcm(boundary_lengths(256)[item], item, BOUNDARY_SEEDS[item])


@functools.lru_cache(maxsize=None)
def boundary_batch(pcm16=False, H=256):
    """(x [4, max], lengths): item b is one signal on the int16 grid -- at hop 120 its first H (T - 1) + r samples --, behind it NaN (fp32)
    or -32768 (int16)"""
    lengths = boundary_lengths(H)
    x = np.full((4, max(lengths)), -32768, dtype=np.int16) if pcm16 else np.full((4, max(lengths)), np.nan, dtype=np.float32)
    for b, L in enumerate(lengths):
        v = _boundary_pcm(b)[:L]
        x[b, :L] = v if pcm16 else v.astype(np.float32) / np.float32(ST.MAX_WAV)
    x.setflags(write=False)
    return x, np.asarray(lengths, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def boundary_reference(pcm16=False, H=256, W=1024):
    """per item: (mc [T, ORDER] float64, the smallest power cell)"""
    x, lengths = boundary_batch(pcm16, H)
    out = []
    for b, L in enumerate(lengths):
        P = power(x[b, :L], H, W)
        out.append((mel_cepstrum_of_log_power(np.log(P)), float(P.min())))
    return out


@functools.lru_cache(maxsize=None)
def boundary_yardstick(pcm16=False, H=256, W=1024):
    """max |fp32 yardstick - float64 reference| over boundary_batch (CPU)"""
    from efficient_tts_amd.mcep import mcep_table
    table32 = mcep_table(N, ORDER, ALPHA).astype(np.float32)
    x, lengths = boundary_batch(pcm16, H)
    ref = boundary_reference(pcm16, H, W)
    return max(float(np.abs(yardstick_item(x[b, :L], H, W, table32).astype(np.float64) - ref[b][0]).max()) for b, L in enumerate(lengths))


DIST_COUNTS = (1023, 1024, 1025, 2049, 5)     # n = min(Ta, Tb) per pair
DIST_DIMS = (ORDER + 1, ORDER)                # with and without c~[0]


def dist_frames(D, seed=0):
    """(x fp32 [B, Tx, D], x_frames, y fp32 [B, Ty, D], y_frames): cepstrum-like rows (coefficient k falls off as 1 / (1 + k)), y a disturbed
    copy whose disturbance grows along the item; the shorter side alternates; NaN in the rows at and beyond each count"""
    rng = np.random.default_rng(seed + D)
    B, T = len(DIST_COUNTS), max(DIST_COUNTS) + 3
    x = np.full((B, T, D), np.nan, dtype=np.float32)
    y = np.full((B, T + 2, D), np.nan, dtype=np.float32)
    xf, yf = [], []
    for b, n in enumerate(DIST_COUNTS):
        ta, tb = (n, min(n + 2, T + 2)) if b % 2 == 0 else (min(n + 3, T), n)
        fall = 1.0 / (1.0 + np.arange(D))
        x[b, :ta] = (rng.standard_normal((ta, D)) * fall).astype(np.float32)
        y[b, :tb] = (rng.standard_normal((tb, D)) * fall).astype(np.float32)
        m = min(ta, tb)
        y[b, :m] = (x[b, :m] + np.linspace(0.05, 0.5, m)[:, None] * y[b, :m]).astype(np.float32)
        xf.append(ta)
        yf.append(tb)
    return x, np.asarray(xf, dtype=np.int32), y, np.asarray(yf, dtype=np.int32)
