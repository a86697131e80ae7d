"""The IIR filter's definition (include/efts_abi.h, "IIR filtering of a padded batch") twice over in float64, and the inputs that
tests/test_iir_cpu.py and tests/test_iir_gpu.py share.  Never imports the product.

`sequential` is the definition: one strictly sequential loop, sample by sample from sample 0, no blocks.  `block_carry` restates the
kernels' scheme -- Z per segment from zero state, M^(2^k) from the recurrence itself, the scan over chunks of 64 segments in the header's
order, then every segment again from its start state -- with numpy's separately rounded products and sums where the device folds an fma."""
import functools

import numpy as np

L = 256                                        # EFTS_IIR_SEGMENT (tests/test_iir_cpu.py compares it with the header)
LANES = 64                                     # segments of one chunk of the scan
RATE = 22050
PEAK = 0.5                                     # of the tone plus DC; the bound's absolute term is 1e-10 of it
LENGTHS = (0, 1, L - 1, L, L + 1, LANES * L - 1, LANES * L, LANES * L + 1, 12345, 40000)
N = 40003                                      # samples per row of the batch: odd, so that most rows begin off a 16-byte boundary
IMPULSES = (L - 1, L, LANES * L)
GARBAGE = 1e30                                 # what lies behind every length in the fp32 batch


def sequential(x, sos) -> np.ndarray:
    """float64 [len(x)]: the sections in order on every sample, transposed direct form II from zero state"""
    y = [float(v) for v in x]
    for b0, b1, b2, a1, a2 in (tuple(float(c) for c in row) for row in np.asarray(sos, dtype=np.float64)):
        s1 = s2 = 0.0
        for n, v in enumerate(y):
            o = b0 * v + s1
            s1 = b1 * v - a1 * o + s2
            s2 = b2 * v - a2 * o
            y[n] = o
    return np.array(y, dtype=np.float64)


def _run(sos, state, x):
    """the cascade over the columns of x [steps, lanes] from `state` [2K, lanes] (changed in place); returns y [steps, lanes]"""
    y = np.empty_like(x)
    for n in range(x.shape[0]):
        v = x[n]
        for q, (b0, b1, b2, a1, a2) in enumerate(sos):
            o = b0 * v + state[2 * q]
            state[2 * q] = b1 * v - a1 * o + state[2 * q + 1]
            state[2 * q + 1] = b2 * v - a2 * o
            v = o
        y[n] = v
    return y


def powers(sos) -> np.ndarray:
    """float64 [6, 2K, 2K]: column i of entry k is the state after 2^k L zero-input steps from the unit state e_i"""
    sos = np.asarray(sos, dtype=np.float64)
    n = 2 * sos.shape[0]
    state, out = np.eye(n), []
    for k in range(6):
        _run(sos, state, np.zeros((L if k == 0 else L * 2 ** (k - 1), n)))
        out.append(state.copy())
    return np.stack(out)


def block_carry(x, sos, m=None) -> np.ndarray:
    """float64 [len(x)]: the same filter by launches A, B and C of the header"""
    sos = np.asarray(sos, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    n, length = 2 * sos.shape[0], len(x)
    nseg = -(-length // L)
    if nseg == 0:
        return np.zeros(0)
    m = powers(sos) if m is None else m
    seg = np.zeros((nseg * L,))
    seg[:length] = x
    seg = seg.reshape(nseg, L).T                                           # [L, nseg]
    z = np.zeros((n, nseg))
    _run(sos, z, seg)                                                      # A
    z[:, [s for s in range(nseg) if (s + 1) * L >= length]] = 0.0          # (only a full segment with a successor has a Z)
    start = np.zeros((n, nseg))
    carry = np.zeros(n)
    for c in range(0, nseg, LANES):                                        # B
        p = np.zeros((n, LANES))
        p[:, :min(LANES, nseg - c)] = z[:, c:c + LANES]
        for i in range(n):
            acc = p[i, 0]
            for j in range(n):
                acc = m[0][i, j] * carry[j] + acc
            p[i, 0] = acc
        for k in range(6):
            d, before = 2 ** k, p.copy()
            for i in range(n):
                acc = before[i, d:].copy()
                for j in range(n):
                    acc = m[k][i, j] * before[j, :-d] + acc
                p[i, d:] = acc
        chunk = np.concatenate([carry[:, None], p[:, :-1]], axis=1)
        start[:, c:c + LANES] = chunk[:, :min(LANES, nseg - c)]
        carry = p[:, -1].copy()
    return _run(sos, start, seg).T.reshape(-1)[:length]                    # C


@functools.lru_cache(maxsize=None)
def signal() -> np.ndarray:
    """float32 [N]: a 220 Hz tone of amplitude 0.4, modulated at 3 Hz, on a DC offset of 0.1 (peak 0.5), plus unit impulses at L - 1, L, 64 L"""
    t = np.arange(N, dtype=np.float64) / RATE
    x = 0.4 * np.sin(2 * np.pi * 220.0 * t) * (0.6 + 0.4 * np.cos(2 * np.pi * 3.0 * t)) + 0.1
    assert np.abs(x).max() <= PEAK
    for i in IMPULSES:
        x[i] += 1.0
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def batch(pcm16: bool = False):
    """(audio [10, N] float32 | int16, lengths int32 [10]): row b is the signal times (1 - b / 40), cut at its length.  fp32: GARBAGE behind every length.  int16: the rounded, clipped samples, -12345 behind."""
    rows = np.stack([signal() * np.float32(1.0 - b / 40.0) for b in range(len(LENGTHS))]).astype(np.float32)
    lengths = np.array(LENGTHS, dtype=np.int32)
    if pcm16:
        a = np.clip(np.round(rows.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
        for b, n in enumerate(LENGTHS):
            a[b, n:] = -12345
        return a, lengths
    for b, n in enumerate(LENGTHS):
        rows[b, n:] = GARBAGE
    return rows, lengths


def twin(pcm: np.ndarray) -> np.ndarray:
    """the fp32 batch that the int16 batch is read as: (float) sample * (1 / 32768), exact"""
    return pcm.astype(np.float32) * np.float32(1.0 / 32768.0)


def bound(ref: np.ndarray) -> np.ndarray:
    """what |device - reference| may be, element by element: one fp32 ulp of the reference, and 1e-10 of the peak near zero"""
    return 2.0 ** -23 * np.abs(ref) + 1e-10 * PEAK


@functools.lru_cache(maxsize=None)
def _reference(sos_bytes: bytes, sections: int):
    sos = np.frombuffer(sos_bytes, dtype=np.float64).reshape(sections, 5)
    audio, lengths = batch(False)
    return tuple(sequential(audio[b, :n], sos) for b, n in enumerate(lengths))


def reference(sos):
    """the sequential float64 output of every item of the fp32 batch, computed once per filter"""
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    return _reference(sos.tobytes(), sos.shape[0])
