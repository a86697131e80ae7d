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


# ---- the inputs of tests/test_audio_boundaries_*.py: items past one workgroup of launch A (F frames), past one turn of launch B's strided
# loops (256 frames) and past one workgroup of launch C (TR_COPY outputs)
SCAN_TURN, COPY_BLOCK = 256, 4096             # TR_THREADS (csrc/efts_trim_energy.h:11), TR_COPY (csrc/efts_trim_energy.h:15)
# a hop of 202 = 2 (mod 8): with it start = (first sound frame - keep_frames) * H is no multiple of 4 for an odd frame, which no hop of PAIRS
# can give
BOUNDARY_PAIRS = PAIRS + [(1024, 202)]
BOUNDARY_KEEP = 0
BOUNDARY_NAMES = ("energy_full", "energy_plus_1", "first_sound_past_turn", "last_sound_past_turn", "copy_4095", "copy_4096", "copy_4097", "copy_8293",
                  "short")


def energy_frames(W, H):
    """F of tr_launch_energy (csrc/efts_trim_energy.h:106): the frames of one workgroup of launch A"""
    return max(1, min(64, (12288 - W) // H + 1))


def _shape(rng, n, lead, burst_end):
    """int16 [n]: uniform noise 45 dB under the burst, the burst (amplitude 20000) over [lead, burst_end), the low level again"""
    low = 20000.0 * 10.0 ** (-45.0 / 20.0)
    amp = np.full(n, low)
    amp[lead:burst_end] = 20000.0
    return np.round(rng.uniform(-1.0, 1.0, size=n) * amp).astype(np.int16)


def boundary_items(W, H, dtype=np.int16, seed=4242):
    """(x [9, ld_in], lengths): the items of BOUNDARY_NAMES, full scale (32767) behind every item; ld_in = 3 (mod 8): no row but the first
    is aligned.  fp32: the same integers times 2^-15, exact.
    energy_full / energy_plus_1: F H and F H + 1 samples, the burst from 3 / 8 of the item to its end, and the item's largest sample (30000)
    is its last: with keep_frames = 0 the last frame decides new_len and the last hop chunk the gain; in energy_plus_1 both belong to the
    second workgroup of launch A.
    first_sound_past_turn: 262 hops of the low level -- noise, not zeros --, a burst of 3 hops, 2 hops of the low level.
    last_sound_past_turn: 3 hops of the low level, the burst up to hop 260, 6 hops of the low level and 5 samples.
    copy_N: 6 hops and 3 samples of the low level, then the burst to the item's end, which lies N samples behind `start`."""
    rng = np.random.default_rng(seed + W + H)
    F = energy_frames(W, H)
    rows = []
    for n in (F * H, F * H + 1):
        rows.append(_shape(rng, n, 3 * n // 8, n))
        rows[-1][-1] = 30000
    rows.append(_shape(rng, 267 * H, 262 * H, 265 * H))
    rows.append(_shape(rng, 266 * H + 5, 3 * H, 260 * H))
    for new_len in (4095, 4096, 4097, 8293):
        full = _shape(rng, 6 * H + 3 + 9000, 6 * H + 3, 6 * H + 3 + 9000)
        start = trim(full, W=W, H=H, keep_frames=BOUNDARY_KEEP)["start"]
        rows.append(full[:start + new_len])
    rows.append(_shape(rng, 1000, 400, 600))
    lengths = [len(v) for v in rows]
    ld_in = max(lengths) + 3
    ld_in += (3 - ld_in) % 8
    x = np.full((len(rows), ld_in), 32767, dtype=np.int16)
    for b, v in enumerate(rows):
        x[b, :len(v)] = v
    if dtype != np.int16:
        x = (x.astype(np.float32) * np.float32(2.0 ** -15)).astype(np.float32)
    return x, tuple(lengths)
