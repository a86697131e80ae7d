"""numpy-only restatement of the silence trimmer's definition (include/efts_abi.h, "Silence trimming and peak normalisation"), and the
inputs that the CPU and GPU tests share.  It never sees the product's code.

int16: energies are Python / int64 integers, the decision is the one float64 multiply and compare of the definition -- exact.
fp32: energies are float64 sums of the float64 squares; the decision margin says how far every frame is from the threshold.
"""
import numpy as np

PAIRS = [(1024, 256), (512, 128), (2048, 512), (1024, 200)]          # (W, H); the last hop does not divide the frame
LENGTHS = (4001, 0, 2500, 1024, 256, 37)                             # the row of length 0 is loud padding throughout, right behind the longest
LD_IN = 4003                                                          # no multiple of 4 or 8
TOP_DB = 40.0
OTHER = ((30.0, 0), (50.0, 0), (40.0, 1), (40.0, 9))                 # (top_db, keep_frames) at W, H = 1024, 256: 30 dB cuts the 35 dB items as well


def ratio(top_db):
    return float(10.0 ** (np.float64(top_db) / 10.0))


def trim(x, W=1024, H=256, top_db=TOP_DB, keep_frames=2, peak=None, max_wav_value=32768.0, trimming=True):
    """x: one item, int16 or float32 [len].  Returns dict(start, new_len, gain float32, out float32 [new_len], margin_db, energies)."""
    x = np.asarray(x)
    pcm = x.dtype == np.int16
    assert pcm or x.dtype == np.float32
    n = int(x.shape[0])
    pad = (W - H) // 2
    assert W in (512, 1024, 2048) and 1 <= H <= W and (W - H) % 2 == 0
    T = -(-n // H)
    r = ratio(top_db)
    sq = x.astype(np.int64) ** 2 if pcm else x.astype(np.float64) ** 2
    padded = np.concatenate([np.zeros(pad + W, sq.dtype), sq, np.zeros(pad + W + H, sq.dtype)])
    energies = [padded[pad + W + t * H - pad: pad + W + t * H - pad + W].sum() for t in range(T)]
    energies = [int(e) for e in energies] if pcm else [float(e) for e in energies]
    e_max = max(energies) if T else 0
    margin = np.inf
    sound = []
    for t, e in enumerate(energies):
        if e_max > 0 and np.float64(e) * np.float64(r) > np.float64(e_max):
            sound.append(t)
        if e_max > 0 and e > 0:
            margin = min(margin, abs(10.0 * np.log10(np.float64(e) * r / np.float64(e_max))))
    start, end, gain = 0, n, np.float32(1.0)
    if e_max > 0:
        if trimming:
            start = max(0, (sound[0] - keep_frames) * H)
            end = min(n, (sound[-1] + 1 + keep_frames) * H)
        kept = x[start:end]
        p = int(np.abs(kept.astype(np.int64)).max()) if pcm else np.float32(np.abs(kept).max())
        if peak is not None and p > 0:
            gain = np.float32(peak) / np.float32(p)
        else:
            gain = np.float32(1.0 / max_wav_value) if pcm else np.float32(1.0)
    out = x[start:end].astype(np.float32) * np.float32(gain)
    return dict(start=start, new_len=end - start, gain=np.float32(gain), out=out.astype(np.float32), margin_db=float(margin), energies=energies)


def items(dtype=np.int16, seed=2027):
    """[B, LD_IN]: per item leading low-level noise, a louder burst, trailing low-level noise; full scale (32767) behind every item's length.
    The burst is uniform noise of amplitude 20000; the low level lies 45 dB under it on items 0, 3, 5 (with top_db 40 the edges are 5 dB under the
    threshold: trimmed) and 35 dB under it on items 2, 4 (5 dB over: kept).  fp32: the same integers times 2^-15, exact."""
    rng = np.random.default_rng(seed)
    x = np.full((len(LENGTHS), LD_IN), 32767, dtype=np.int16)
    for b, n in enumerate(LENGTHS):
        low = 20000.0 * 10.0 ** ((-45.0 if b in (0, 3, 5) else -35.0) / 20.0)
        lead, burst = 3 * n // 8, n // 4
        amp = np.concatenate([np.full(lead, low), np.full(burst, 20000.0), np.full(n - lead - burst, low)])
        x[b, :n] = np.round(rng.uniform(-1.0, 1.0, size=n) * amp).astype(np.int16)
    if dtype == np.int16:
        return x
    return (x.astype(np.float32) * np.float32(2.0 ** -15)).astype(np.float32)
