"""numpy-only restatement of the pause shortener's definition (include/efts_abi.h, "Shortening the long pauses INSIDE the items"), and the
inputs that the CPU and GPU tests share.  It never sees the product's code.

int16: energies are Python / int64 integers, the decision is the one float64 multiply and compare of the definition -- exact.
fp32: energies are float64 sums of the float64 squares; `margin_db` says how far every frame is from the threshold.
Runs are found in a plain loop over the chunks, the copy goes sample by sample, the fade is taken in float64 from the fp32 table and the
fp32 difference.
"""
import os
import re

import numpy as np

TOP_DB = 40.0
RATE = 22050


def plan_tile():
    """the chunks that the plan kernel walks at a time: the constant that the kernel is compiled with"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "efts_abi.h")) as handle:
        return int(re.search(r"#define EFTS_PAUSES_TILE (\d+)", handle.read()).group(1))


def ratio(top_db):
    return float(10.0 ** (np.float64(top_db) / 10.0))


def fade_table(F):
    return np.array([np.float32((np.float64(k) + 0.5) / np.float64(F)) for k in range(F)], dtype=np.float32)


def pause_chunks(max_pause_ms, rate, H):
    return max(1, int(round(max_pause_ms * rate / (1000.0 * H))))


def sound_flags(x, W, H, top_db=TOP_DB):
    """(flags [T], margin_db) of one item, int16 or float32"""
    x = np.asarray(x)
    pcm = x.dtype == np.int16
    assert pcm or x.dtype == np.float32
    assert W in (512, 1024, 2048) and 1 <= H <= W and (W - H) % 2 == 0
    n = int(x.shape[0])
    pad = (W - H) // 2
    T = -(-n // H)
    r = ratio(top_db)
    sq = x.astype(np.int64) ** 2 if pcm else x.astype(np.float64) ** 2
    padded = np.concatenate([np.zeros(pad, sq.dtype), sq, np.zeros(W + H, sq.dtype)])
    energies = [padded[t * H: t * H + W].sum() for t in range(T)]
    energies = [int(e) for e in energies] if pcm else [float(e) for e in energies]
    e_max = max(energies) if T else 0
    margin = np.inf
    flags = []
    for e in energies:
        flags.append(bool(e_max > 0 and np.float64(e) * np.float64(r) > np.float64(e_max)))
        if e_max > 0 and e > 0:
            margin = min(margin, abs(10.0 * np.log10(np.float64(e) * r / np.float64(e_max))))
    return flags, float(margin)


def plan(flags, M):
    """(keep [T] of bool, joints {source chunk in front of a joint: the chunk c1 - tail that the fade runs into}, runs [(c0, c1)] of all pauses)"""
    T = len(flags)
    keep = [True] * T
    joints, runs = {}, []
    sound = [t for t in range(T) if flags[t]]
    if not sound:
        return keep, joints, runs
    t_first, t_last = sound[0], sound[-1]
    head, tail = (M + 1) // 2, M // 2
    c = t_first + 1
    while c <= t_last:
        if flags[c]:
            c += 1
            continue
        c0 = c
        while not flags[c]:                                  # (ends at t_last at the latest)
            c += 1
        c1 = c
        runs.append((c0, c1))
        if c1 - c0 > M:
            for d in range(c0 + head, c1 - tail):
                keep[d] = False
            joints[c0 + head - 1] = c1 - tail
    return keep, joints, runs


def shorten(x, W=1024, H=256, top_db=TOP_DB, M=26, F=64, max_wav_value=32768.0):
    """x: one item, int16 or float32 [len].  Returns dict(new_len, removed, pauses, chunk_src [list], out float64 [new_len] (exact outside
    the fades, the float64 fade value inside), is_fade bool [new_len], margin_db, runs, flags)."""
    x = np.asarray(x)
    n = int(x.shape[0])
    assert 0 <= F <= H and M >= 1
    flags, margin = sound_flags(x, W, H, top_db)
    keep, joints, runs = plan(flags, M)
    xf = x.astype(np.float32) * np.float32(1.0 / max_wav_value) if x.dtype == np.int16 else x       # one fp32 multiply per sample
    w = fade_table(F)
    out, is_fade, chunk_src = [], [], []
    for c in range(len(flags)):
        if not keep[c]:
            continue
        chunk_src.append(c)
        for k in range(H):
            i = c * H + k
            if i >= n:
                break
            kk = k - (H - F)
            if c in joints and kk >= 0:
                xa, xb = xf[i], xf[joints[c] * H - F + kk]
                out.append(np.float64(xa) + np.float64(w[kk]) * np.float64(np.float32(xb) - np.float32(xa)))
                is_fade.append(True)
            else:
                out.append(np.float64(xf[i]))
                is_fade.append(False)
    removed = H * sum(1 for k in keep if not k)
    assert len(out) == n - removed
    return dict(new_len=n - removed, removed=removed, pauses=len(joints), chunk_src=chunk_src, out=np.array(out, dtype=np.float64),
                is_fade=np.array(is_fade, dtype=bool), margin_db=margin, runs=runs, flags=flags)


# ---- the inputs of the GPU tests: tone bursts at 0.5 with gaps of noise 60 dB down

def overhang(W, H):
    """(before, after): the chunks in front of / behind a burst on whole chunks whose frames still touch it, and are sound with it"""
    pad = (W - H) // 2
    return -(-(W + H) // (2 * H)) - 1, -(-pad // H)


def layout(spec, W, H):
    """tone ranges [(first chunk, end chunk)] from a list of ("noise", k) | ("tone", k) | ("tone_until", chunk) | ("quiet", run length):
    "quiet" leaves so many chunks of noise that `run length` of them are quiet when a burst follows"""
    before, after = overhang(W, H)
    pos, tones = 0, []
    for op, val in spec:
        if op == "noise":
            pos += val
        elif op == "tone":
            tones.append((pos, pos + val))
            pos += val
        elif op == "tone_until":
            assert val > pos
            tones.append((pos, val))
            pos = val
        else:
            assert op == "quiet"
            pos += val + before + after
    return tones


def render(tones, n, H, dtype, seed):
    """one item of n samples: a 0.5 sine on the tone chunks, uniform noise of amplitude 0.0005 elsewhere, as int16 (rounded) or as the same
    integers times 2^-15 in float32"""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.float64)
    x = rng.uniform(-1.0, 1.0, size=n) * 0.0005
    tone = 0.5 * np.sin(2.0 * np.pi * i / 97.3)
    for s, e in tones:
        x[s * H:e * H] = tone[s * H:e * H]
    pcm = np.round(x * 32768.0).astype(np.int16)
    return pcm if dtype == np.int16 else (pcm.astype(np.float32) * np.float32(2.0 ** -15)).astype(np.float32)


LENGTHS = (0, 1, 255, 256, 257, 12345, 40000, 70000)


def specs(W, H, tile):
    """the layouts of LENGTHS: the short items are one burst; 12 345: a long quiet lead-in and tail; 40 000: a lead-in gap of one chunk, runs
    around every M of the tests; 70 000 (for H = 64: 1 094 chunks): pauses across the first, second and third boundary of the plan's tile"""
    short = [("tone", 2)]
    mid = [("noise", 12), ("tone", 3), ("quiet", 1), ("tone", 3), ("quiet", 8), ("tone", 3)]
    long_ = [("noise", 1), ("tone", 3)]
    for run in (1, 2, 3, 7, 8, 12, 20):
        long_ += [("quiet", run), ("tone", 3)]
    before, after = overhang(W, H)
    huge = [("noise", 1), ("tone", 6), ("quiet", 1), ("tone", 5), ("quiet", 2), ("tone", 5), ("quiet", 7), ("tone", 5), ("quiet", 8),
            ("tone_until", tile - 5 - after), ("quiet", 12), ("tone", 5), ("quiet", 3), ("tone_until", 2 * tile - 3 - after), ("quiet", 6), ("tone", 6),
            ("quiet", tile + 44), ("tone", 5)]
    return [short, short, short, short, short, mid, long_, huge]


def batch(W, H, dtype, tile, count=len(LENGTHS), seed=2031):
    """[count, n]: the first `count` items of LENGTHS in rows of the longest one's length rounded up to 8; full scale behind every item"""
    lengths = LENGTHS[:count]
    n = -(-max(lengths) // 8) * 8
    x = np.full((count, n), 32767 if dtype == np.int16 else 32767.0 * 2.0 ** -15, dtype=dtype)
    for b, (length, spec) in enumerate(zip(lengths, specs(W, H, tile))):
        x[b, :length] = render(layout(spec, W, H), length, H, dtype, seed + b)
    return x, lengths
