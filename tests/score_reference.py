"""Float64 numpy restatement of the scorer (efficient_tts_amd/score.py, csrc/efts_score.hip), written from the definitions and never importing
the product's tables.

    table[k-1][n] = sqrt(2 / N) cos(pi k (n + 1/2) / N), k = 1 .. n_coef           (orthonormal DCT-II without row 0)
    d(i, j) = sqrt(sum_k (x_i[k] - y_j[k])^2)
    A(0, 0) = d(0, 0), L(0, 0) = 1;  A(i, j) = d(i, j) + A(p), L(i, j) = 1 + L(p), p the cheapest existing predecessor among
    (i-1, j-1), (i-1, j), (i, j-1) in this order, a later one replacing an earlier one only when strictly smaller
    cost = A(Tx-1, Ty-1), path_len = L(Tx-1, Ty-1)

`dtw` also returns the on-path margin: the smallest gap between the best and the runner-up predecessor over the cells of its own optimal
path (cells with a single predecessor have none), divided by cost.  While the margin exceeds the relative error of an fp32 evaluation,
that evaluation takes the same path.
"""
import math

import numpy as np

MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)


def table(n_mels: int, n_coef: int) -> np.ndarray:
    out = np.empty((n_coef, n_mels), dtype=np.float64)
    for k in range(1, n_coef + 1):
        for n in range(n_mels):
            out[k - 1, n] = math.sqrt(2.0 / n_mels) * math.cos(math.pi * k * (n + 0.5) / n_mels)
    return out


def mel_cepstrum(mel: np.ndarray, n_coef: int) -> np.ndarray:
    """[T, n_mels] -> [T, n_coef], float64"""
    return np.asarray(mel, dtype=np.float64) @ table(mel.shape[1], n_coef).T


def gamma(tx: int, ty: int, d: int) -> float:
    """relative bound on the cost of an fp32 evaluation: every local cost carries at most about D + 3 roundings, a path adds at most
    Tx + Ty - 1 more, all terms are positive; the factor 2 covers second-order terms"""
    return 2.0 * (tx + ty + d + 3) * 2.0 ** -24


def dtw(x: np.ndarray, y: np.ndarray):
    """(cost, path_len, on-path margin) of x [Tx, D] against y [Ty, D] (the fp32 inputs cast to float64); one anti-diagonal per step"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    tx, ty = x.shape[0], y.shape[0]
    d2 = np.zeros((tx, ty))
    for k in range(x.shape[1]):
        d2 += (x[:, k, None] - y[None, :, k]) ** 2
    d = np.sqrt(d2)
    # cell (i, j) lives at [i + 1, j + 1]; the border is +inf except the cell in front of (0, 0), which is (0, length 0)
    A = np.full((tx + 1, ty + 1), np.inf)
    A[0, 0] = 0.0
    Ln = np.zeros((tx + 1, ty + 1), dtype=np.int64)
    choice = np.zeros((tx, ty), dtype=np.int8)
    for s in range(tx + ty - 1):
        i = np.arange(max(0, s - ty + 1), min(s, tx - 1) + 1)
        j = s - i
        best, ln, c = A[i, j].copy(), Ln[i, j].copy(), np.zeros(i.shape[0], dtype=np.int8)
        for code, (a, l) in ((1, (A[i, j + 1], Ln[i, j + 1])), (2, (A[i + 1, j], Ln[i + 1, j]))):
            m = a < best
            best[m], ln[m], c[m] = a[m], l[m], code
        A[i + 1, j + 1], Ln[i + 1, j + 1], choice[i, j] = d[i, j] + best, ln + 1, c
    cost = float(A[tx, ty])
    i, j, gap = tx - 1, ty - 1, np.inf
    while (i, j) != (0, 0):
        cands = sorted(v for v in (A[i, j], A[i, j + 1], A[i + 1, j]) if np.isfinite(v))
        if len(cands) > 1:
            gap = min(gap, cands[1] - cands[0])
        i, j = ((i - 1, j - 1), (i - 1, j), (i, j - 1))[choice[i, j]]
    return cost, int(Ln[tx, ty]), (gap / cost if cost > 0 else np.inf)
