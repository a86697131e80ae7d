"""GPU (-m gpu): the warping path of `score.dtw_path` (efts_dtw_path) and its consumers against tests/pitch_reference.py.

Shapes sit on each side of the kernel's boundaries, derived from DTW_THREADS = 256 lanes, DTW_ROWS = 4 rows per lane and DTW_BAND = 1024
rows per band: Tx around one lane's rows (3, 4, 5), around one and two bands (1023, 1024, 1025, 2049); Ty around the ring refill and the
back-trace windows (255, 256, 257, 513).  Batched raggedly, NaN behind every length, the path pre-filled with a poison value.

Exact inputs (D = 1, small integers): every distance and every partial sum is exact in fp32 and float64 alike, ties are everywhere and resolve
identically, so path, path_len and cost must EQUAL the reference.  Real-valued inputs (D = 13): the path must be valid, the float64 sum of the
distances along it within (path_len + D + 4) 2^-23 of cost, and cost and path_len bit-equal to efts_dtw's.
"""
import math

import numpy as np
import pytest
import torch

import pitch_reference as P
from efficient_tts_amd import lib as L
from efficient_tts_amd import score as S

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (3, 2), (4, 255), (5, 256), (1023, 257), (1024, 513), (1025, 2), (2049, 255), (1, 513), (1024, 1), (5, 513), (1025, 257)]
BATCHES = [PAIRS[0:4] + PAIRS[8:11], PAIRS[4:6], PAIRS[6:8] + PAIRS[11:12]]
POISON = -77


@pytest.fixture(scope="module")
def dev():
    L.load()
    L.require_device()
    return torch.device("cuda:0")


def _batch(dev, xs, ys):
    """(x, x_lengths, y, y_lengths) on the device: NaN beyond every length"""
    def pad(items):
        T = max(max(v.shape[0] for v in items), 1)
        buf = np.full((len(items), T, items[0].shape[1]), np.nan, dtype=np.float32)
        for b, v in enumerate(items):
            buf[b, :v.shape[0]] = v
        return torch.from_numpy(buf).to(dev), torch.tensor([v.shape[0] for v in items], dtype=torch.int32, device=dev)
    return (*pad(xs), *pad(ys))


def _run_poisoned(dev, x, xl, y, yl):
    """efts_dtw_path with every output pre-filled, so that what the kernel leaves alone can be seen"""
    B, Tx, D = x.shape
    Ty = y.shape[1]
    lib = L.load()
    ws = torch.empty(B * lib.efts_dtw_path_workspace_bytes(Tx, Ty), dtype=torch.uint8, device=dev)
    cost = torch.full((B,), -7.0, dtype=torch.float32, device=dev)
    plen = torch.full((B,), -1, dtype=torch.int32, device=dev)
    path = torch.full((B, Tx + Ty - 1, 2), POISON, dtype=torch.int32, device=dev)
    L.check(lib.efts_dtw_path(x.data_ptr(), x.stride(1), x.stride(0), xl.data_ptr(), Tx, y.data_ptr(), y.stride(1), y.stride(0), yl.data_ptr(), Ty, D,
                              cost.data_ptr(), plen.data_ptr(), path.data_ptr(), ws.data_ptr(), ws.numel(), B, torch.cuda.current_stream().cuda_stream),
            "efts_dtw_path")
    torch.cuda.synchronize()
    return cost.cpu().numpy(), plen.cpu().numpy(), path.cpu().numpy()


@pytest.mark.parametrize("n", range(len(BATCHES)))
def test_exact_inputs_equal_the_reference(dev, n):
    rng = np.random.default_rng(300 + n)
    xs = [rng.integers(-2, 3, size=(tx, 1)).astype(np.float32) for tx, _ in BATCHES[n]]
    ys = [rng.integers(-2, 3, size=(ty, 1)).astype(np.float32) for _, ty in BATCHES[n]]
    cost, plen, path = _run_poisoned(dev, *_batch(dev, xs, ys))
    for b, (x, y) in enumerate(zip(xs, ys)):
        ref_cost, ref_len, ref_path = P.dtw_path_reference(x, y)
        assert float(cost[b]) == ref_cost and int(plen[b]) == ref_len, (x.shape, y.shape)
        assert np.array_equal(path[b, :ref_len], ref_path), (x.shape, y.shape)
        assert (path[b, ref_len:] == POISON).all()


@pytest.mark.parametrize("n", range(len(BATCHES)))
def test_real_valued_inputs(dev, n):
    D = 13
    rng = np.random.default_rng(400 + n)
    xs = [np.cumsum(rng.normal(size=(tx, D)), axis=0).astype(np.float32) for tx, _ in BATCHES[n]]
    ys = [np.cumsum(rng.normal(size=(ty, D)), axis=0).astype(np.float32) for _, ty in BATCHES[n]]
    x, xl, y, yl = _batch(dev, xs, ys)
    cost, plen, path = _run_poisoned(dev, x, xl, y, yl)
    cost0, plen0 = S.dtw(x, xl, y, yl)
    assert np.array_equal(cost0.cpu().numpy().view(np.uint32), cost.view(np.uint32)) and np.array_equal(plen0.cpu().numpy(), plen)
    for b, (xv, yv) in enumerate(zip(xs, ys)):
        tx, ty, k = xv.shape[0], yv.shape[0], int(plen[b])
        assert max(tx, ty) <= k <= tx + ty - 1
        assert P.path_is_valid(path[b, :k], tx, ty), (tx, ty)
        assert (path[b, k:] == POISON).all()
        cells = path[b, :k]
        along = float(np.sqrt(((xv.astype(np.float64)[cells[:, 0]] - yv.astype(np.float64)[cells[:, 1]]) ** 2).sum(axis=1)).sum())
        bound = (k + D + 4) * 2.0 ** -23
        rel = abs(along - float(cost[b])) / along
        print(f"{tx} x {ty}: path_len {k}, cost {float(cost[b])!r}, float64 sum along the path {along!r}: {rel:.3e} = {rel / bound:.3f} of the bound")
        assert rel <= bound


def test_empty_and_mixed_items(dev):
    rng = np.random.default_rng(9)
    xs = [rng.integers(-2, 3, size=(t, 1)).astype(np.float32) for t in (7, 0, 5, 300)]
    ys = [rng.integers(-2, 3, size=(t, 1)).astype(np.float32) for t in (9, 4, 0, 260)]
    cost, plen, path = _run_poisoned(dev, *_batch(dev, xs, ys))
    for b in (1, 2):
        assert math.isnan(cost[b]) and plen[b] == 0 and (path[b] == POISON).all()
    for b in (0, 3):
        ref_cost, ref_len, ref_path = P.dtw_path_reference(xs[b], ys[b])
        assert float(cost[b]) == ref_cost and int(plen[b]) == ref_len and np.array_equal(path[b, :ref_len], ref_path)


def test_f0_error_on_hand_built_contours(dev):
    n = 300                                                            # more cells than one pass of the kernel's 256 lanes
    diag = np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.int32)
    base = 100.0 + np.arange(n, dtype=np.float32)
    cases = []
    cases.append((base, base * np.float32(1.1), diag, n))                                         # all voiced
    cases.append((base, np.zeros(n, np.float32), diag, n))                                        # no voiced pair: NaN, every cell differs
    b = base.copy()
    b[10:47] = 0.0                                                                                 # voicing differs on 37 cells
    cases.append((base, b, diag, n))
    cases.append((base, base * np.float32(2.0), diag, n))                                          # an octave: exactly 1200 cents
    cases.append((base, base, diag, 0))                                                            # an empty path
    rng = np.random.default_rng(4)
    _, k, warped = P.dtw_path_reference(rng.normal(size=(150, 1)), rng.normal(size=(151, 1)))      # a real path, shorter than the buffer
    wp = np.full((n, 2), 10 ** 6, dtype=np.int32)                                                  # cells behind path_len point far outside
    wp[:k] = warped
    a = np.where(rng.random(n) < 0.7, base, 0.0).astype(np.float32)
    c = np.where(rng.random(n) < 0.7, base * np.float32(1.25), 0.0).astype(np.float32)
    cases.append((a, c, wp, k))
    f0_a = torch.from_numpy(np.stack([c_[0] for c_ in cases])).to(dev)
    f0_b = torch.from_numpy(np.stack([c_[1] for c_ in cases])).to(dev)
    path = torch.from_numpy(np.stack([c_[2] for c_ in cases])).to(dev)
    plen = torch.tensor([c_[3] for c_ in cases], dtype=torch.int32, device=dev)
    out = {k_: v.cpu().numpy() for k_, v in S.F0Error(dev)(f0_a, f0_b, path, plen).items()}
    # fp32 against float64: the ratio's rounding (2^-24) moves log2 by 2^-24 / ln 2 = 8.6e-8, log2f adds about as much; against log2 1.1 = 0.1375
    # that is 1.3e-6 relative, the fused sum and the square root add a few 2^-24: 1e-5 leaves a factor of five
    for i, (a_, b_, p_, k_) in enumerate(cases):
        rmse, vuv, pairs = P.f0_error_reference(a_, b_, p_[:k_])
        assert int(out["voiced_pairs"][i]) == pairs, i
        for got, want in ((out["f0_rmse_cents"][i], rmse), (out["vuv_error"][i], vuv)):
            assert (math.isnan(want) and math.isnan(got)) or got == pytest.approx(want, rel=1e-5), (i, got, want)
    assert math.isnan(out["f0_rmse_cents"][1]) and out["vuv_error"][1] == 1.0 and out["voiced_pairs"][2] == n - 37
    assert out["vuv_error"][2] == pytest.approx(37 / n, rel=1e-6) and abs(float(out["f0_rmse_cents"][3]) - 1200.0) <= 1e-3
    assert out["voiced_pairs"][4] == 0 and math.isnan(out["vuv_error"][4])


def test_mcd_with_the_path_keeps_every_bit(dev):
    rng = np.random.default_rng(12)
    mel_a = torch.from_numpy(rng.normal(size=(3, 70, 80)).astype(np.float32)).to(dev)
    mel_b = torch.from_numpy(rng.normal(size=(3, 90, 80)).astype(np.float32)).to(dev)
    la, lb = torch.tensor([70, 33, 0], device=dev), torch.tensor([81, 90, 50], device=dev)
    scorer = S.MelCepstralDistortion(dev)
    plain = scorer(mel_a, la, mel_b, lb)
    with_path = scorer(mel_a, la, mel_b, lb, return_path=True)
    assert set(with_path) == set(plain) | {"path"} and tuple(with_path["path"].shape) == (3, 70 + 90 - 1, 2)
    for key in ("mcd", "cost", "path_len", "frames_ratio"):
        a, b = plain[key].cpu().numpy(), with_path[key].cpu().numpy()
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), key
    for b in range(2):
        k = int(with_path["path_len"][b])
        assert P.path_is_valid(with_path["path"][b, :k].cpu().numpy(), int(la[b]), int(lb[b]))
    assert int(with_path["path_len"][2]) == 0
